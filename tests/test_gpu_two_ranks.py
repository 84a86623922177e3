"""The category-partitioned multi-GPU evaluation with REAL kernels and more
than one rank: the ranks share the one GPU of the test box and talk over gloo
(RCCL refuses two ranks on one device), so pack -> all-gather -> unpack runs
between genuinely different processes holding different category blocks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import orclib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


# `which`: "synth", or "predrules" -- the prediction-rule set of
# tests/predrules.py (test_gpu_pred_rules.py), evaluated under its max_dets
MAX_DETS = {"synth": 300, "predrules": 8}


def _rule_set():
    import predrules
    return predrules.sized(max_dets=MAX_DETS["predrules"]).columns()


def _problem(world, which="synth"):
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns, GTColumns
    from tao_amodal_amd.synth import synth
    if which == "predrules":
        gt, dt = _rule_set()
    else:
        parts = [synth(seed=23 + r, V=4, F=20, C=40, dets_per_frame=30, n_present=5,
                       video_id_base=r * 4) for r in range(world)]
        gt = GTColumns.concat([p[0] for p in parts])
        dt = DTColumns.concat([p[1] for p in parts])
    fl = flatten.flatten_lvis(gt, dt, MAX_DETS[which])
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    return fl, flatten.flatten_tao(gt, dt, MAX_DETS[which])


def _join(rank, world, port):
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)


def _worker(rank, world, port, out, which="synth"):
    _join(rank, world, port)
    _category_rank(rank, world, out, which)
    dist.destroy_process_group()


def _category_rank(rank, world, out, which):
    from tao_amodal_amd import dist as tdist, engine
    fl, ft = _problem(world, which)
    dev = torch.device("cuda", 0)
    k0, k1, _ = tdist.category_block(len(fl.cat_ids), rank, world)
    plan = tdist.CategoryPlan(
        engine.DeviceProblem(tdist.shard_by_category(fl, k0, k1), dev),
        engine.DeviceProblem(tdist.shard_by_category(ft, k0, k1), dev),
        rank, world, dev)
    plan.step()
    plan.step()
    torch.cuda.synchronize()
    plan.lvis.check()
    plan.tao.check()
    torch.save({"lvis": (plan.lvis.precision.cpu().numpy(), plan.lvis.recall.cpu().numpy()),
                "tao": (plan.tao.precision.cpu().numpy(), plan.tao.recall.cpu().numpy())},
               os.path.join(out, "r%d.pt" % rank))


def _spawn(worker, world, *args):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(worker, args=(world, port) + args, nprocs=world, join=True)


def check_category_plan(tmp_path, world, which, spawn=True):
    if spawn:
        _spawn(_worker, world, str(tmp_path), which)
    fl, ft = _problem(world, which)
    want = {"lvis": orclib.run_flat(fl, detail=False),
            "tao": orclib.run_flat(ft, detail=False)}
    for rank in range(world):
        got = torch.load(os.path.join(str(tmp_path), "r%d.pt" % rank), weights_only=False)
        for k in ("lvis", "tao"):
            assert np.array_equal(got[k][0], want[k]["precision"]), (rank, k)
            assert np.array_equal(got[k][1], want[k]["recall"]), (rank, k)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharing_one_gpu_reproduce_the_whole_problem(tmp_path, world):
    check_category_plan(tmp_path, world, "synth")


# --------------------------------------------------------------------------
# By-video plan, a rank WITHOUT a detection in its own category block (ADVICE
# r5): the rank's own-block slices of the send buffers are empty -- a NULL data
# pointer -- while records of the other rank arrive for that very block.
# --------------------------------------------------------------------------
def _unit_parts(world, which="synth"):
    from tao_amodal_amd.synth import synth
    if which == "predrules":
        # the `ties` video alone on rank 0 (among its own images the tied tracks
        # come in another order than among all: check_video_plan), the others
        # dealt out to the remaining ranks
        gt, dt = _rule_set()
        rank_of = {int(v): 0 if k == 0 else 1 + (k - 1) % (world - 1)
                   for k, v in enumerate(np.sort(gt.vid_id))}
        return [(gt.select_videos([rank_of[int(v)] == r for v in gt.vid_id]),
                 dt.take(np.flatnonzero([rank_of[int(v)] == r for v in dt.video_id])))
                for r in range(world)]
    parts = [synth(seed=61 + r, V=3, F=12, C=40, dets_per_frame=25, n_present=6,
                   video_id_base=r * 3) for r in range(world)]
    # the last rank keeps only detections of the FIRST owner's categories
    gt, dt = parts[-1]
    kb = (40 + world - 1) // world
    first_block = np.sort(np.asarray(gt.cat_id))[:kb]
    parts[-1] = (gt, dt.take(np.flatnonzero(np.isin(dt.category_id, first_block))))
    return parts


def _unit_worker(rank, world, port, out, which="synth"):
    _join(rank, world, port)
    _video_rank(rank, world, out, which)
    dist.destroy_process_group()


def _both_worker(rank, world, port, out, which):
    """Both plans in one process group: <out>/category, <out>/video."""
    _join(rank, world, port)
    _category_rank(rank, world, os.path.join(out, "category"), which)
    _video_rank(rank, world, os.path.join(out, "video"), which)
    dist.destroy_process_group()


def _cells_of(f, unit_ids, field):
    """{(unit id, category id): the cell's rows of `field`}"""
    unit, cat = np.asarray(f["cell_unit"]), np.asarray(f["cell_cat"])
    off, col = np.asarray(f["cell_dt_off"]), np.asarray(f[field])
    return {(int(unit_ids[unit[k]]), int(f.cat_ids[cat[k]])): col[off[k]:off[k + 1]].tolist()
            for k in range(f.n_cells)}


def _video_rank(rank, world, out, which):
    from tao_amodal_amd import dist as tdist, engine, flatten, flatten_dev
    dev = torch.device("cuda", 0)
    gt, dt = _unit_parts(world, which)[rank]
    universe = tdist.gather_visit_universe(gt, dev)
    f_l = flatten_dev.flatten_lvis(gt, dt, MAX_DETS[which], device=dev)
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    f_t = flatten_dev.flatten_tao(gt, dt, MAX_DETS[which], device=dev, visit_universe=universe)
    # the rank's own tables: the detections of every cell, in order
    tables = {"lvis": _cells_of(f_l, f_l.img_ids, "dt_score"),
              "tao": _cells_of(f_t, f_t.vid_ids, "dt_id")}
    plan = tdist.ExchangePlan(engine.DeviceProblem(f_l, dev), engine.DeviceProblem(f_t, dev),
                              rank, world, dev)
    empty_own = [ev.own_at >= ev.dp.n_dt and ev.n_recv > 0 for ev in (plan.lvis, plan.tao)]
    plan.step()
    plan.step()
    torch.cuda.synchronize()
    plan.lvis.check()
    plan.tao.check()
    torch.save({"lvis": (plan.lvis.precision.cpu().numpy(), plan.lvis.recall.cpu().numpy()),
                "tao": (plan.tao.precision.cpu().numpy(), plan.tao.recall.cpu().numpy()),
                "empty_own": empty_own, "tables": tables},
               os.path.join(out, "r%d.pt" % rank))


def check_video_plan(tmp_path, world, which, spawn=True):
    from tao_amodal_amd import flatten
    from tao_amodal_amd.columns import DTColumns, GTColumns
    parts = _unit_parts(world, which)
    if which == "predrules":
        # the case is really hit: by rank 0's own images the tied tracks come in
        # another order than by the images of all ranks (visit_universe)
        import predrules
        rule_set = predrules.sized(max_dets=MAX_DETS[which])
        own = predrules.tie_order(rule_set, flatten.video_images(parts[0][0]))
        assert own != predrules.tie_order(rule_set, flatten.video_images(
            GTColumns.concat([p[0] for p in parts])))
    if spawn:
        _spawn(_unit_worker, world, str(tmp_path), which)
    gt = GTColumns.concat([p[0] for p in parts])
    dt = DTColumns.concat([p[1] for p in parts])
    fl = flatten.flatten_lvis(gt, dt, MAX_DETS[which])
    dt.track_id, _ = flatten.make_track_ids_unique(dt)
    ft = flatten.flatten_tao(gt, dt, MAX_DETS[which])
    want = {"lvis": orclib.run_flat(fl, detail=False), "tao": orclib.run_flat(ft, detail=False)}
    whole = {"lvis": _cells_of(fl, fl.img_ids, "dt_score"), "tao": _cells_of(ft, ft.vid_ids, "dt_id")}
    for rank in range(world):
        got = torch.load(os.path.join(str(tmp_path), "r%d.pt" % rank), weights_only=False)
        # the rank's tables = the whole set's cells of its videos / images
        units = {"lvis": set(parts[rank][0].img_id.tolist()),
                 "tao": set(parts[rank][0].vid_id.tolist())}
        for k in ("lvis", "tao"):
            assert got["tables"][k] == {c: v for c, v in whole[k].items()
                                        if c[0] in units[k]}, (rank, k)
        if rank == world - 1 and which == "synth":
            assert all(got["empty_own"]), got["empty_own"]     # (the case is really hit)
        for k in ("lvis", "tao"):
            assert np.array_equal(got[k][0], want[k]["precision"]), (rank, k)
            assert np.array_equal(got[k][1], want[k]["recall"]), (rank, k)


@pytest.mark.timeout(600)
def test_by_video_rank_without_detections_in_its_own_block(tmp_path):
    check_video_plan(tmp_path, 2, "synth")


def check_both_plans(tmp_path, world, which):
    """check_category_plan and check_video_plan on ranks spawned once."""
    for sub in ("category", "video"):
        os.makedirs(os.path.join(str(tmp_path), sub))
    _spawn(_both_worker, world, str(tmp_path), which)
    check_category_plan(os.path.join(str(tmp_path), "category"), world, which, spawn=False)
    check_video_plan(os.path.join(str(tmp_path), "video"), world, which, spawn=False)
