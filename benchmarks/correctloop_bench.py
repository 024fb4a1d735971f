#!/usr/bin/env python3
"""Device CorrectLoop on one MI355X (csrc/orbx_correctloop.hip).

    python benchmarks/correctloop_bench.py [--steps 3] [--warmup 1] [--repeats 5] [--loop-kf 1400]
                                           [--out profiles/correctloop_bench.json]

The 1400-keyframe loop map of covis_bench.py / culling_bench.py (global_ba_model.make_banded: a
closed path, a covisibility band, 8 new points per keyframe) with the loop closed at its last
keyframe: cur = the last keyframe, loop = the 31st, mg2oScw = cur's pose moved by a few degrees and
4 % of scale; the fusion gives cur and its two best neighbours 12 points each of the loop keyframe
and of its two successors.  Timed, interleaved, `repeats` windows of `steps` calls after `warmup`
calls (the optimiser: one call a window), each window closed by a device synchronise; the median is
reported with min and max:
  propagate            orbx_correct_loop_propagate_device (net of the state restore timed beside it)
  assemble             orbx_essential_graph_assemble_device (likewise)
  update_normal_depth  orbx_update_normal_and_depth_device over every MapPoint
  optimize             orbx_optimize_essential_graph_batch_device on the assembled tables (B = 1)
  host_edges           the wall time of the host essential_graph_edges on the same inputs (lists built
                       from the graph read back to the host; building them is not in the figure)
The device edges are checked against the host's.  One JSON line, also written to --out.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "benchmarks"))

LOOP_SHAPE = dict(window=6, pts_per_kf=8, n_loop=40, kind="mixed")


def bench_map(loop_kf):
    """kf_mp, poses and octaves by keyframe id along the path, the points, cur (the last keyframe),
    loop (the 31st) and the id of every path position."""
    import global_ba_model as G
    from covis_bench import scene_map
    loop = G.make_banded(800, loop_kf, **LOOP_SHAPE)
    by_slot = scene_map(loop)
    slot = np.asarray(loop["slot"])
    # keyframe ids along the path (the scene's keypoint rows are shuffled): the envelope that the
    # optimiser factors follows the ids, and mnId grows along the trajectory
    kf_mp = np.ascontiguousarray(by_slot[slot])
    octave = np.ascontiguousarray(np.asarray(loop["kps_oct"], np.int32)[slot])
    n = len(slot)
    return kf_mp, np.asarray(loop["Tcw"], np.float32), np.asarray(loop["pos"], np.float32), octave, n - 1, 30, np.arange(n)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="correctloop_bench.py")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-kf", type=int, default=1400)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "correctloop_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import correct_loop_model as M
    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LoopCorrector
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer, essential_graph_edges

    if not torch.cuda.is_available():
        raise SystemExit("correctloop_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    kf_mp, poses, pos, octave, cur, loop, slot = bench_map(args.loop_kf)
    K, cap = kf_mp.shape
    n_mp, max_conn, min_feat = len(pos), 64, 12
    kf_n = np.full(K, cap, np.int32)
    zero_k, zero_n = np.zeros(K, np.uint8), np.zeros(n_mp, np.uint8)
    st = M.with_geometry(kf_mp, kf_n, zero_k, zero_n, 3, poses=poses, mp_pos=pos, octave=octave)
    Scw = M.drift_scw(st, cur, 9)
    keys = np.zeros((K, cap), L.KEYPOINT_DTYPE)
    keys["octave"] = st["octave"]
    g = CovisibilityGraph(K, cap, n_mp, max_conn=max_conn)
    d_kf_mp, d_kfn, d_kf_bad, d_mp_bad = t(kf_mp), t(kf_n), t(zero_k), t(zero_n)
    d = {"kf_Tcw": t(st["poses"]), "mp_pos": t(st["mp_pos"]), "mp_corrected_by_kf": t(st["mp_corrected_by_kf"]),
         "mp_corrected_ref": t(st["mp_corrected_ref"]), "mp_ref_kf": t(st["mp_ref_kf"]),
         "kf_keys_un": t(keys.view(np.uint8).reshape(K, cap * 28)).view(K, cap, 28), "normal": t(st["normal"]),
         "max_distance": t(st["max_distance"]), "min_distance": t(st["min_distance"])}
    mutable = ("kf_Tcw", "mp_pos", "mp_corrected_by_kf", "mp_corrected_ref", "normal", "max_distance", "min_distance")
    saved0 = {k: d[k].clone() for k in mutable}
    d_Scw = t(Scw)
    all_ids = np.arange(K, dtype=np.int32)
    lc = LoopCorrector(g, d, st["scale"])
    # the loop edges of earlier closures: the far-reaching pairs of essgraph_bench.py
    n = args.loop_kf
    pairs = [(int(slot[a]), int(slot[b])) for a, b in ((n - 200, n // 3), (n // 2, n // 8), (n // 4, 10))]
    loops = {k: [] for k in range(K)}
    for a, b in pairs:
        loops[a].append(b)
        loops[b].append(a)
    off = np.zeros(K + 1, np.int32)
    ids = []
    for k in range(K):
        ids += sorted(loops[k])
        off[k + 1] = len(ids)
    d_loop_off, d_loop_ids = t(off), t(np.array(ids, np.int32))

    def note(msg):
        print(f"[correctloop_bench] {msg}", file=sys.stderr, flush=True)

    def refresh(table):
        g.refresh_observations(table, d_kfn, d_kf_bad, d_mp_bad, stream=stream)

    def restore_a():  # the state before the propagation
        for k, v in saved0.items():
            d[k].copy_(v)
        refresh(d_kf_mp)
        g.update_connections(all_ids, stream=stream)

    def propagate():
        restore_a()
        lc.propagate(cur, Scw=d_Scw, stream=stream)

    propagate()
    torch.cuda.synchronize(dev)
    note("first propagation")
    p = lc.state()
    n_conn = int(p["n_conn"][0])
    conn = p["conn"][:n_conn].copy()
    takers = [cur] + [int(k) for k in conn[:2]]
    donors = [loop] + [int(k) for k in g.ordered(loop)[0][:2]]
    km = kf_mp.copy()
    for k in takers:  # room for the fusion
        km[k, np.flatnonzero(km[k] >= 0)[-3 * 12:]] = -1
    d_kf_mp.copy_(t(km))
    d_fused = t(M.fuse(km, kf_n, takers, donors, 12, seed=3))
    propagate()  # again on the table with room
    torch.cuda.synchronize(dev)
    saved1 = {k: d[k].clone() for k in mutable}
    p = lc.state()
    n_conn = int(p["n_conn"][0])
    conn = p["conn"][:n_conn].copy()
    corrected = int((d["mp_corrected_by_kf"] == cur).sum())

    def restore_b():  # the state after the propagation, the fusion and the refresh
        for k, v in saved1.items():
            d[k].copy_(v)
        refresh(d_kf_mp)
        g.update_connections(all_ids, stream=stream)
        g.update_connections(conn, stream=stream)
        refresh(d_fused)

    max_edges = K * 16

    def assemble():
        restore_b()
        lc.assemble(loop, d_loop_off, d_loop_ids, min_feat, max_edges=max_edges, max_lc=4096, stream=stream)

    assemble()
    torch.cuda.synchronize(dev)
    a = lc.state()
    assert int(a["status"][0]) == 0, int(a["status"][0])
    n_rows, n_edges, blocks = int(a["n_rows"][0]), int(a["n_edges"][0]), int(a["env_blocks"][0])
    note(f"assembled: {n_rows} vertices, {n_edges} edges, {blocks} envelope blocks")
    if blocks > 40 * n_rows:  # one workgroup factors the envelope: a near-dense one takes minutes per solve
        raise SystemExit(f"correctloop_bench.py: the envelope has {blocks} blocks for {n_rows} vertices; not timing the optimiser")
    opt = EssentialGraphOptimizer()

    def optimize():
        lc.optimize(opt, fix_scale=True, max_env_blocks=blocks, stream=stream)

    def normal_depth():
        lc.update_normal_and_depth(stream=stream)

    # the host form's inputs from the graph read back, and its wall time
    gs = g.state()
    rows = [k for k in range(K)]
    parent = gs["parent"].tolist()
    children = {k: [] for k in rows}
    for c, par in enumerate(parent):
        if par >= 0:
            children[par].append(c)
    covis = [list(zip(gs["ordered_kf"][k, :gs["ordered_n"][k]].tolist(), gs["ordered_w"][k, :gs["ordered_n"][k]].tolist()))
             for k in rows]
    lco = a["lc_off"]
    lcs = [(int(a["lc_member"][r]), list(zip(a["lc_kf"][lco[r]:lco[r + 1]].tolist(), a["lc_w"][lco[r]:lco[r + 1]].tolist())))
           for r in range(n_conn)]
    host_args = (rows, parent, [children[k] for k in rows], [sorted(loops[k]) for k in rows], covis, lcs, cur, loop, min_feat)
    ev, kind = essential_graph_edges(*host_args)
    assert np.array_equal(ev, a["edge_v"][:n_edges]) and np.array_equal(kind, a["edge_kind"][:n_edges])
    host_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        essential_graph_edges(*host_args)
        host_ms.append((time.perf_counter() - t0) * 1e3)

    runs = {"restore_a": restore_a, "propagate": propagate, "restore_b": restore_b, "assemble": assemble,
            "update_normal_depth": normal_depth, "optimize": optimize}
    steps = {name: 1 if name == "optimize" else args.steps for name in runs}  # the optimiser runs for a long time
    for name, fn in runs.items():
        for _ in range(max(1, args.warmup)):
            fn()
        torch.cuda.synchronize(dev)
        note(f"warmed {name}")
    times = {name: [] for name in runs}
    for _ in range(args.repeats):
        for name, fn in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps[name]):
                fn()
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) / steps[name])
    note("timed")
    r = {}
    for name, v in times.items():
        ms = sorted(1e3 * x for x in v)
        r[name] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
    o = lc.state()
    opt.close()
    prop = round(r["propagate"]["ms_per_call"] - r["restore_a"]["ms_per_call"], 4)
    asm = round(r["assemble"]["ms_per_call"] - r["restore_b"]["ms_per_call"], 4)
    opt_ms = r["optimize"]["ms_per_call"]
    out = {"metric": f"ms CorrectLoop's propagation + essential-graph assembly, {args.loop_kf}-keyframe loop map",
           "value": round(prop + asm, 4), "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "higher_is_better": False, "data": "synthetic",
           "map": {"keyframes": args.loop_kf, "rows": K, "cap": cap, "mappoints": n_mp, "max_conn": max_conn, "cur": cur,
                   "loop": loop, "members": n_conn, "corrected_points": corrected, "loop_connections": int(lco[n_conn]),
                   "vertices": n_rows, "edges": n_edges, "kind0_edges": int((kind == 0).sum()), "envelope_blocks": blocks,
                   "min_feat": min_feat},
           **r, "propagate_ms_net": prop, "assemble_ms_net": asm,
           "optimize_trace": o["trace"].reshape(-1).tolist(), "optimize_status": int(o["status"][0]),
           "share_of_optimize": {"propagate": round(prop / opt_ms, 4), "assemble": round(asm / opt_ms, 4),
                                 "update_normal_depth": round(r["update_normal_depth"]["ms_per_call"] / opt_ms, 4)},
           "host_edges_ms": {"median": round(statistics.median(host_ms), 4), "min": round(min(host_ms), 4),
                             "max": round(max(host_ms), 4)},
           "not_measured": ["a recorded sequence's map (the shapes are synthetic)", "the reference on a CPU",
                            "the host form's list building and the copies it needs", "the global histogram path at this size"]}
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
