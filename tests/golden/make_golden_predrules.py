"""Record what the REFERENCE's class API does with the prediction-rule sets of
tests/predrules.py under max_dets 3 and 8 (the CLI cannot pass max_dets, and
it stops at the clash inputs).  Runs only in the development container (needs
/root/reference, see refenv.py).  Writes, next to F11's golden files:

  f11/predrules.npz       per set (m3, m8) and side (lvis, tao): precision /
                          recall restricted to the categories that are not all
                          -1; the prediction list after LVISResults /
                          TaoResults rewrote it in place, by input position:
                          id (0: cut away), score, area (NaN: cut away),
                          category_id; the post-cut list as input positions;
                          required_average
  f11/predrules.json.gz   the ragged parts: per track id score / len / area /
                          frame image ids / input position of the box kept per
                          frame; track_scores; per (video, category) cell the
                          track ids in the order of compute_iou; per clash
                          input (predrules.clash_inputs) the exception's type
                          and message, None where the reference accepts it

Usage:  python tests/golden/make_golden_predrules.py
"""
import copy
import gzip
import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))
sys.path.insert(2, os.path.dirname(os.path.dirname(HERE)))
import predrules  # noqa: E402
import refenv  # noqa: E402

AVERAGE_WARNING = "At least one track had annotations with different scores"


def valid(p):
    return np.flatnonzero((p.reshape(p.shape[0], p.shape[1], p.shape[2], -1) > -1)
                          .any(axis=(0, 1, 3)))


def rewritten(preds, post, out, key):
    """The caller's dicts after the constructor, by input position."""
    nan = float("nan")
    out[key + "_id"] = np.array([p.get("id", 0) for p in preds], dtype=np.int64)
    out[key + "_score"] = np.array([p["score"] for p in preds], dtype=np.float64)
    out[key + "_area"] = np.array([p.get("area", nan) for p in preds], dtype=np.float64)
    out[key + "_category_id"] = np.array([p["category_id"] for p in preds], dtype=np.int64)
    at = {id(p): i for i, p in enumerate(preds)}
    out[key + "_post_cut"] = np.array([at[id(p)] for p in post], dtype=np.int64)


def record_set(name, ref_lvis, ref_tao, work, arrays, ragged):
    s = predrules.recorded_set(name)
    gt_path = os.path.join(work, name + "_gt.json")
    with open(gt_path, "w") as f:
        json.dump(s.gt, f)
    # ---- image level
    preds = copy.deepcopy(s.preds)
    res = ref_lvis.LVISResults(gt_path, preds, max_dets=s.max_dets)
    rewritten(preds, res.dataset["annotations"], arrays, name + "_lvis")
    le = ref_lvis.LVISEval(gt_path, res, "bbox")
    le.run()
    p, r = le.eval["precision"], le.eval["recall"]
    k = valid(p)
    arrays.update({name + "_lvis_valid_k": k, name + "_lvis_precision": p[:, :, k],
                   name + "_lvis_recall": r[:, k], name + "_lvis_shape": np.array(p.shape)})
    # ---- track level
    preds = copy.deepcopy(s.preds)
    warned = []

    class H(logging.Handler):
        def emit(self, record):
            warned.append(record.getMessage())
    lg = logging.getLogger("tao.results")
    lg.handlers, lg.propagate = [H()], False
    lg.setLevel(logging.INFO)
    res = ref_tao.TaoResults(ref_tao.Tao(gt_path), preds, max_dets=s.max_dets)
    arrays[name + "_required_average"] = np.array(
        any(w.startswith(AVERAGE_WARNING) for w in warned))
    rewritten(preds, res.dataset["annotations"], arrays, name + "_tao")
    te = ref_tao.TaoEval(ref_tao.Tao(gt_path), res, logger=logging.getLogger("golden.pr"))
    te.logger.propagate = False
    te.run()
    p, r = te.eval["precision"], te.eval["recall"]
    k = valid(p)
    arrays.update({name + "_tao_valid_k": k, name + "_tao_precision": p[:, :, k],
                   name + "_tao_recall": r[:, k], name + "_tao_shape": np.array(p.shape)})
    at = {id(q): i for i, q in enumerate(preds)}
    tracks, cells = {}, []
    for (v, c), dts in sorted(te._dts.items()):
        if not dts:
            continue
        for d in dts:
            kept = {}
            for a in d["annotations"]:      # the dict of compute_iou: the last one wins,
                kept[a["image_id"]] = at[id(a)]     # an image keeps its first place
            tracks[str(d["id"])] = {"score": float(d["score"]), "len": len(d["annotations"]),
                                    "area": float(d["area"]), "video_id": int(d["video_id"]),
                                    "category_id": int(d["category_id"]),
                                    "frame_images": [int(i) for i in kept],
                                    "frame_boxes": list(kept.values())}
        e = te.eval_vids[te.params.vid_ids.index(v), te.params.cat_ids.index(c), 0, 0]
        cells.append({"key": [int(v), int(c)], "dt_ids": [int(x) for x in e["dt_ids"]]})
    ragged[name] = {
        "tracks": tracks, "cells": cells,
        "track_scores": {str(t): float(x["score"]) for t, x in res.tracks.items()}}
    # ---- inputs the reference rejects
    clash = {}
    for cname, cpreds in predrules.clash_inputs(s).items():
        clash[cname] = {}
        for side, make in (
                ("lvis", lambda q: ref_lvis.LVISResults(gt_path, q, max_dets=s.max_dets)),
                ("tao", lambda q: ref_tao.TaoResults(ref_tao.Tao(gt_path), q,
                                                     max_dets=s.max_dets))):
            try:
                make(copy.deepcopy(cpreds))
                clash[cname][side] = None
            except Exception as e:
                clash[cname][side] = [type(e).__name__, str(e)]
    ragged[name]["clash"] = clash
    print(name, len(s.preds), "boxes", len(tracks), "tracks with a row",
          {c: v["tao"] and v["tao"][0] for c, v in clash.items()})


def main():
    ref_lvis, ref_tao = refenv.import_reference()
    logging.getLogger().setLevel(logging.CRITICAL)
    work = "/tmp/golden_predrules"
    os.makedirs(work, exist_ok=True)
    arrays, ragged = {}, {}
    for name in predrules.RECORDED:
        record_set(name, ref_lvis, ref_tao, work, arrays, ragged)
    out = os.path.join(HERE, "f11")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "predrules.npz"), **arrays)
    with gzip.GzipFile(os.path.join(out, "predrules.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(ragged, separators=(",", ":"), sort_keys=True).encode())
    print({f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))})


if __name__ == "__main__":
    main()
