#!/usr/bin/env python3
"""LocalMapping's culls on one MI355X (csrc/orbx_culling.hip).

    python benchmarks/culling_bench.py [--steps 3] [--warmup 1] [--repeats 5] [--loop-kf 1400]
                                       [--recent 2000] [--out profiles/culling_bench.json]

On globalba_bench.py's synthetic loop map of --loop-kf keyframes, connected by one batch of
UpdateConnections, with octaves drawn at random (so that nothing is culled) and, for the forced
case, the first candidate of the current keyframe's list doctored to octave 7 (every other
observer passes the scale test: it is culled, and the walk counts the rest itself).  Measured,
each the median of `repeats` interleaved repeats of `steps` calls (min and max beside it), in one
session, with the copy that restores the state timed beside it and subtracted:
  keyframe_culling, nothing culled, the speculative form and "cull_serial"
  keyframe_culling with the forced cull, both forms
  map_point_culling of --recent recent points
  observation_counts
  the observation refresh and UpdateConnections of one keyframe, to set them against.
The reference cannot be built for timing here, so there is no CPU figure.  One JSON line, also
written to --out.
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


def bench_map(loop_kf, seed=5):
    """The loop map's table with the per-keypoint columns the culls read.  Returns kf_mp, octave,
    u_right, the current keyframe (the middle of the loop)."""
    import global_ba_model as G
    from covis_bench import scene_map
    loop = G.make_banded(800, loop_kf, **LOOP_SHAPE)
    kf_mp = scene_map(loop)
    rng = np.random.default_rng(seed)
    octave = rng.integers(0, 8, kf_mp.shape).astype(np.int32)
    u_right = np.where(rng.random(kf_mp.shape) < 0.5, 50.0, -1.0).astype(np.float32)
    return kf_mp, octave, u_right, int(np.asarray(loop["slot"])[loop_kf // 2]), len(loop["pos"])


def main(argv=None):
    ap = argparse.ArgumentParser(prog="culling_bench.py")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-kf", type=int, default=1400)
    ap.add_argument("--recent", type=int, default=2000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "culling_bench.json"))
    args = ap.parse_args(argv)

    import torch

    from orbslam2commentedbyxcm_amd import CovisibilityGraph, MapCuller
    from orbslam2commentedbyxcm_amd import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("culling_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def timed(runs):
        for fn in runs.values():
            for _ in range(max(1, args.warmup)):
                fn()
        times = {name: [] for name in runs}
        for _ in range(args.repeats):
            for name, fn in runs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize(dev)
                times[name].append((time.perf_counter() - t0) / args.steps)
        out = {}
        for name, v in times.items():
            ms = sorted(1e3 * x for x in v)
            out[name] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
        return out

    kf_mp, octave, u_right, cur, n_mp = bench_map(args.loop_kf)
    K, cap = kf_mp.shape
    keys = np.zeros((K, cap), L.KEYPOINT_DTYPE)
    keys["octave"] = octave
    g = CovisibilityGraph(K, cap, n_mp, max_conn=64)
    d_kfn = t(np.full(K, cap, np.int32))
    d = {"kf_mp": t(kf_mp), "kf_bad": torch.zeros(K, dtype=torch.uint8, device=dev),
         "mp_bad": torch.zeros(n_mp, dtype=torch.uint8, device=dev),
         "kf_keys_un": t(keys.view(np.uint8).reshape(K, cap * 28)).view(K, cap, 28), "kf_u_right": t(u_right)}
    saved = {k: d[k].clone() for k in ("kf_mp", "kf_bad", "mp_bad")}

    def refresh():
        g.refresh_observations(d["kf_mp"], d_kfn, d["kf_bad"], d["mp_bad"], stream=stream)

    refresh()
    g.update_connections(np.arange(K, dtype=np.int32), stream=stream)
    cull = MapCuller(g, d)
    cand, _ = g.ordered(cur)
    victim = int(next(k for k in cand if k != 0))
    keys_forced = keys.copy()
    keys_forced["octave"][victim] = 7
    d_keys = {"none": d["kf_keys_un"], "forced": t(keys_forced.view(np.uint8).reshape(K, cap * 28)).view(K, cap, 28)}

    def restore_tables():
        for k, v in saved.items():
            d[k].copy_(v)

    def restore_graph():  # after a cull: the tables, the observations, and the victim's connections
        restore_tables()
        refresh()
        g.update_connections([victim], stream=stream)

    def culling(keys_name, serial, restore):
        def fn():
            restore()
            cull.tables["kf_keys_un"] = d_keys[keys_name]
            L.debug_set("cull_serial", serial)
            cull.keyframe_culling(cur, True, stream=stream)
            L.debug_set("cull_serial", -1)
        return fn

    def update_one():
        g.update_connections([cur], stream=stream)

    d_out = torch.zeros(n_mp, dtype=torch.int32, device=dev)

    def obs_counts():
        cull.observation_counts(d_out, stream=stream)

    rng = np.random.default_rng(9)
    n_recent = min(args.recent, n_mp)
    recent = rng.permutation(n_mp)[:n_recent].astype(np.int32)
    visible = rng.integers(1, 9, n_mp).astype(np.int32)
    found = np.minimum(rng.integers(0, 9, n_mp), visible).astype(np.int32)
    first = rng.integers(6, 11, n_mp).astype(np.int32)
    d_recent0, d_recent, d_nrec = t(recent), t(recent), t(np.array([n_recent], np.int32))
    d_first, d_found, d_visible = t(first), t(found), t(visible)

    def restore_mp():
        restore_tables()
        d_recent.copy_(d_recent0)
        d_nrec.fill_(n_recent)
        refresh()

    def mp_cull():
        restore_mp()
        cull.map_point_culling(10, True, d_recent, d_nrec, d_first, d_found, d_visible, stream=stream)

    # what each case does, once
    culling("none", 0, restore_tables)()
    st = cull.state()
    nc = int(st["n_cand"][0])
    none = {"candidates": nc, "culled": int(st["n_culled"][0]), "mean_nMPs": round(float(st["cand_counts"][:nc, 0].mean()), 1)}
    culling("forced", 0, restore_graph)()
    st = cull.state()
    forced = {"victim_position": int(np.flatnonzero(cand == victim)[0]), "culled": int(st["n_culled"][0]),
              "new_bad_mappoints": int(st["n_new_bad_mp"][0])}
    mp_cull()
    torch.cuda.synchronize(dev)
    mp = {"recent": n_recent, "kept": int(d_nrec[0]), "culled": int(cull.state()["n_mp_culled"][0])}
    restore_graph()

    r = timed({"restore_tables": restore_tables, "restore_graph": restore_graph, "restore_mp": restore_mp,
               "cull_none_speculative": culling("none", 0, restore_tables), "cull_none_serial": culling("none", 1, restore_tables),
               "cull_forced_speculative": culling("forced", 0, restore_graph), "cull_forced_serial": culling("forced", 1, restore_graph),
               "map_point_culling": mp_cull, "observation_counts": obs_counts, "refresh_observations": refresh,
               "update_connections_one": update_one})
    net = {}
    for name, base in (("cull_none_speculative", "restore_tables"), ("cull_none_serial", "restore_tables"),
                       ("cull_forced_speculative", "restore_graph"), ("cull_forced_serial", "restore_graph"),
                       ("map_point_culling", "restore_mp")):
        net[name + "_ms_net"] = round(r[name]["ms_per_call"] - r[base]["ms_per_call"], 4)
    spec, ser = net["cull_none_speculative_ms_net"], net["cull_none_serial_ms_net"]
    out = {"metric": f"ms KeyFrameCulling of one keyframe, nothing culled, {args.loop_kf}-keyframe loop map",
           "value": spec, "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "higher_is_better": False, "dtype": "i32", "data": "synthetic",
           "map": {"keyframes": args.loop_kf, "rows": K, "cap": cap, "mappoints": n_mp, "current_keyframe": cur},
           "nothing_culled": none, "forced_cull": forced, "map_point_culling_case": mp, **r, **net,
           "speculative_minus_serial_ms_nothing_culled": round(spec - ser, 4),
           "note": "every keyframe_culling and map_point_culling figure includes the observation refresh it ends with",
           "not_measured": ["a recorded sequence's map (the shapes are synthetic)",
                            f"candidate lists past this map's {nc}", "the reference on a CPU (it cannot be built for timing here)",
                            "the global histogram path at this size"]}
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    g.close()


if __name__ == "__main__":
    main()
