"""Golden vectors of the reference's own maskApi.c (bbIou and the run-length
mask functions), compiled from the reference source into oracle/_ref by
``__graft_entry__.build()`` (orclib.ref_*).  Writes tests/golden/maskapi/:

    bb_iou.npz       per case <case>_dt, <case>_gt and <case>_iou (bbIou,
                     iscrowd = 0, column-major as the reference returns it)
    bb_iou_domain.npz  per population of tests/boxpop.py <kind>_dt [256, 4],
                     <kind>_gt [96, 4] and <kind>_iou: bbIou on boxes that are
                     any double (NaN sign and payload in the answers are the
                     build machine's and no part of the contract)
    rle.json.gz      "poly": polygons on frames with the reference's
                     rleFrPoly / rleToString / rleFrString / rleToBbox /
                     rleArea answers; "merge": mask lists with the union and
                     intersection of rleMerge and the rleIou matrix
    rle_domain.npz   per pair kind of tests/rlepop.py <kind>_iou (rleIou of
                     each pair), <kind>_inter and <kind>_union (rleArea of
                     rleMerge's intersection and union); answers only, the
                     masks come from the population's seeds

The inputs are the seeded cases the tests ran against the live library; the
masks handed to merge / IoU are rasterised by oracle/rle.py (what the tests
feed it).  Development container only (needs oracle/_ref)."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import boxpop  # noqa: E402
import rlepop  # noqa: E402
import orclib  # noqa: E402
from oracle import rle  # noqa: E402

OUT = os.path.join(HERE, "maskapi")


def _boxes(rng, n, scale):
    return np.ascontiguousarray(
        np.c_[rng.integers(-50, 500, (n, 2)), rng.integers(0, 300, (n, 2))] * scale)


def bb_iou_cases():
    """test_flat_oracle_golden (seed 5, two scales) and the host / device
    bbIou check of test_gpu_parity (seed 3)."""
    cases = {}
    rng = np.random.default_rng(5)
    for name, scale in (("int", 1.0), ("dec", 0.37)):
        dt = _boxes(rng, 200, scale)
        cases[name] = (dt, _boxes(rng, 90, scale))
    rng = np.random.default_rng(3)
    dt = _boxes(rng, 300, 0.37)
    cases["parity"] = (dt, _boxes(rng, 77, 0.37))
    return cases


def _rand_poly(rng, h, w, k=None, spread=0.5):
    k = k or int(rng.integers(3, 9))
    cx, cy = rng.uniform(0, w), rng.uniform(0, h)
    return np.c_[cx + rng.uniform(-w * spread, w * spread, k),
                 cy + rng.uniform(-h * spread, h * spread, k)].ravel()


def poly_cases():
    rng = np.random.default_rng(1)
    out = []
    for it in range(300):
        h, w = int(rng.integers(5, 60)), int(rng.integers(5, 80))
        xy = _rand_poly(rng, h, w, spread=0.7)
        if it % 3 == 0:
            xy = np.round(xy)
        if it % 7 == 0:
            xy[2:4] = xy[0:2]                   # repeated vertex
        a = orclib.ref_rle_fr_poly(xy, h, w)
        s = orclib.ref_rle_to_string(a)
        out.append(dict(h=h, w=w, xy=xy.tolist(), rle=a, string=s,
                        fr_string=orclib.ref_rle_fr_string(s, h, w),
                        bbox=orclib.ref_rle_to_bbox(a),
                        area=orclib.ref_rle_area(a)))
    return out


def merge_cases():
    rng = np.random.default_rng(2)
    out = []
    for it in range(150):
        h, w = int(rng.integers(8, 50)), int(rng.integers(8, 60))
        mk = lambda hh=h: rle.fr_poly(_rand_poly(rng, hh, w).tolist(), hh, w)
        ms = [mk() for _ in range(int(rng.integers(1, 5)))]
        ds, gs = [mk() for _ in range(4)], [mk() for _ in range(3)]
        if it % 10 == 0:
            gs[0] = mk(h + 1)                               # another frame size
        if it % 9 == 0:
            ds[1] = {"h": h, "w": w, "counts": [h * w]}     # empty mask
        if it % 8 == 0:
            ds[2] = {"h": h, "w": w, "counts": [0, h * w]}  # full mask
        out.append(dict(masks=ms, union=orclib.ref_rle_merge(ms, False),
                        intersection=orclib.ref_rle_merge(ms, True),
                        dts=ds, gts=gs, iou=orclib.ref_rle_iou(ds, gs).tolist()))
    return out


def domain_cases():
    arrays = {}
    for kind in rlepop.PAIR_KINDS:
        pairs = rlepop.pairs_of(kind)[0]
        arrays[kind + "_iou"] = np.array([orclib.ref_rle_iou([d], [g])[0, 0] for d, g in pairs])
        for name, cut in (("_inter", True), ("_union", False)):
            arrays[kind + name] = np.array(
                [orclib.ref_rle_area(orclib.ref_rle_merge([d, g], cut)) for d, g in pairs],
                dtype=np.int64)
    return arrays


def main():
    if not os.path.exists(orclib.REF_SO):
        sys.exit("oracle/_ref not built: run __graft_entry__.build() where "
                 "the reference source is present")
    os.makedirs(OUT, exist_ok=True)
    arrays = {}
    for name, (dt, gt) in bb_iou_cases().items():
        arrays[name + "_dt"], arrays[name + "_gt"] = dt, gt
        arrays[name + "_iou"] = orclib.ref_bb_iou(dt, gt)
    np.savez_compressed(os.path.join(OUT, "bb_iou.npz"), **arrays)
    arrays = {}
    for kind in boxpop.KINDS:
        dt, gt = boxpop.golden_boxes(kind)
        arrays[kind + "_dt"], arrays[kind + "_gt"] = dt, gt
        arrays[kind + "_iou"] = orclib.ref_bb_iou(dt, gt)
    np.savez_compressed(os.path.join(OUT, "bb_iou_domain.npz"), **arrays)
    np.savez_compressed(os.path.join(OUT, "rle_domain.npz"), **domain_cases())
    with gzip.open(os.path.join(OUT, "rle.json.gz"), "wt") as f:
        json.dump(dict(poly=poly_cases(), merge=merge_cases()), f)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
