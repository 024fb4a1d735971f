#!/usr/bin/env python3
"""Tracking::UpdateLocalMap on one MI355X (csrc/orbx_localmap.hip).

    python benchmarks/localmap_bench.py [--steps 3] [--warmup 1] [--repeats 5] [--loop-kf 1400]
                                        [--batch 256] [--out profiles/localmap_bench.json]

On globalba_bench.py's synthetic loop map of --loop-kf keyframes, connected by one batch of
UpdateConnections: --batch frames, each at the pose of a keyframe spread along the loop, whose
keypoints are the projections of the MapPoints of a window of 5 neighbouring keyframes; half of
them hold their MapPoint in mvpMapPoints (what the motion-model search leaves), the others are
for SearchLocalPoints to find.  Measured, each the median of `repeats` interleaved repeats (min
and max beside it), in one session:
  update_local_map      orbx_update_local_map_device
  search_local_points   orbx_search_local_points_offsets_device on the lists it produced
  restore               the copy that puts mvpMapPoints back, which both of them include
and the tally.  The shapes are synthetic.  One JSON line, also written to --out.
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
WITH_LOCAL_MAP_STEP_MS = 1.35  # configs[1] + TrackLocalMap, one step of 256 frames


def main(argv=None):
    ap = argparse.ArgumentParser(prog="localmap_bench.py")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-kf", type=int, default=1400)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "localmap_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import global_ba_model as G
    from covis_bench import scene_map
    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LocalMapTracker, ORBmatcher
    from orbslam2commentedbyxcm_amd import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("localmap_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(5)

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

    # ---- the map ----
    loop = G.make_banded(800, args.loop_kf, **LOOP_SHAPE)
    kf_mp = scene_map(loop)
    K, cap = kf_mp.shape
    nk = args.loop_kf
    pos = np.asarray(loop["pos"], np.float32).reshape(-1, 3)
    n_mp = len(pos)
    Tcw = np.asarray(loop["Tcw"], np.float32).reshape(-1, 3, 4)
    slot = np.asarray(loop["slot"])
    fx, fy, cx, cy, bf = (float(v) for v in loop["cam"])
    g = CovisibilityGraph(K, cap, n_mp, max_conn=64)
    d_mp, d_kfn = t(kf_mp), t(np.full(K, cap, np.int32))
    d_bad, d_mpbad = torch.zeros(K, dtype=torch.uint8, device=dev), torch.zeros(n_mp, dtype=torch.uint8, device=dev)
    g.refresh_observations(d_mp, d_kfn, d_bad, d_mpbad, stream=stream)
    g.update_connections(np.arange(K, dtype=np.int32), stream=stream)
    # the MapPoint columns: a random descriptor each; normal and distances from the first observer
    first_kf = np.asarray(loop["obs_kf"])[np.asarray(loop["obs_off"])[:-1]]
    Ow = -np.einsum("kji,kj->ki", Tcw[:, :, :3], Tcw[:, :, 3])
    PO = pos - Ow[first_kf]
    dist = np.linalg.norm(PO, axis=1).astype(np.float32)
    sf = (1.2 ** np.arange(8)).astype(np.float32)
    tab = dict(pos=pos, desc=rng.integers(0, 256, (n_mp, 32)).astype(np.uint8), normal=(PO / dist[:, None]).astype(np.float32),
               max_distance=(dist * sf[2]).astype(np.float32), min_distance=(dist * sf[2] / sf[-1]).astype(np.float32),
               observations=np.diff(np.asarray(loop["obs_off"])).astype(np.int32), bad=np.zeros(n_mp, np.uint8))
    # ---- the frames ----
    B = args.batch
    fm = np.full((B, cap), -1, np.int32)
    kps = np.zeros((B, cap), L.KEYPOINT_DTYPE)
    desc = np.zeros((B, cap, 32), np.uint8)
    n = np.zeros(B, np.int32)
    T = np.zeros((B, 12), np.float32)
    centres = np.linspace(2, nk - 3, B).astype(int)
    for b, c in enumerate(centres):
        T[b] = Tcw[c].reshape(-1)
        pool = np.unique(kf_mp[slot[c - 2:c + 3]])
        pool = pool[pool >= 0]
        Xc = pos[pool] @ Tcw[c, :, :3].T + Tcw[c, :, 3]
        u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        vis = np.flatnonzero((Xc[:, 2] > 0) & (u > 0) & (u < 640) & (v > 0) & (v < 480))
        vis = rng.permutation(vis)[:cap]
        m = len(vis)
        n[b] = m
        kps["x"][b, :m], kps["y"][b, :m] = u[vis], v[vis]
        kps["octave"][b, :m] = 2
        desc[b, :m] = tab["desc"][pool[vis]]
        held = rng.random(m) < 0.5
        fm[b, :m] = np.where(held, pool[vis], -1)
    d_tab = {k: t(v) for k, v in tab.items()}
    d_fm0 = t(fm)
    d_fm = d_fm0.clone()
    d_n, d_T = t(n), t(T)
    d_kps = t(kps.view(np.uint8).reshape(B, cap * 28)).view(B, cap, 28)
    d_desc = t(desc)
    d_nm = torch.zeros((B,), dtype=torch.int32, device=dev)
    max_kf, max_points = 128, 128 * cap
    max_total = B * 4096
    trk = LocalMapTracker(g)
    m = ORBmatcher(0.8, False)
    lm = trk.buffers(B, max_kf, max_total)

    def restore():
        d_fm.copy_(d_fm0)

    def update():
        restore()
        trk.update_local_map(d_fm, d_n, max_kf, max_points, max_total, stream=stream)

    def search():
        restore()
        m.search_local_points_offsets_device(d_tab, d_kps, d_desc, d_n, d_T, lm["local_off"], lm["local_ids"], d_fm, d_nm,
                                             sf, fx, fy, cx, cy, 640, 480, max_local_points=max_points, max_total=max_total,
                                             stream=stream)

    d_out = torch.zeros((B, cap), dtype=torch.uint8, device=dev)

    def tally():
        trk.tally(d_fm, d_n, d_out, d_tab["observations"], stream=stream)

    update()
    search()
    torch.cuda.synchronize(dev)
    st = trk.state()
    held0, after = int((fm >= 0).sum()), int((d_fm.cpu().numpy() >= 0).sum())
    r = timed({"restore": restore, "update_local_map": update, "search_local_points": search, "tally": tally})
    up = r["update_local_map"]["ms_per_call"] - r["restore"]["ms_per_call"]
    se = r["search_local_points"]["ms_per_call"] - r["restore"]["ms_per_call"]
    res = {"map": {"keyframes": nk, "rows": K, "cap": cap, "mappoints": n_mp},
           "frames": {"batch": B, "mean_keypoints": round(float(n.mean()), 1), "mean_held_mappoints": round(held0 / B, 1),
                      "mean_after_search": round(after / B, 1),
                      "mean_local_keyframes": round(float(st["counts"][:, 0].mean()), 1),
                      "max_local_keyframes": int(st["counts"][:, 0].max()),
                      "mean_local_points": round(float(st["counts"][:, 1].mean()), 1),
                      "status_or": int(np.bitwise_or.reduce(st["status"]))},
           **r,
           "update_local_map_ms_net": round(up, 4), "search_local_points_ms_net": round(se, 4),
           "update_share_of_search": round(up / se, 4),
           "with_local_map_step_ms_design_5": WITH_LOCAL_MAP_STEP_MS,
           "update_share_of_with_local_map_step": round(up / WITH_LOCAL_MAP_STEP_MS, 4)}
    out = {"metric": f"frames/s UpdateLocalMap, batch {B}, {nk}-keyframe loop map",
           "value": round(B / (up * 1e-3), 1), "unit": "frames/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "higher_is_better": True, "dtype": "i32", "data": "synthetic", **res,
           "not_measured": ["a recorded sequence's map (the shapes are synthetic: 91 keypoints a frame)",
                            "maps past --loop-kf keyframes", "the split of k_lm_frames between votes, walk and points",
                            "the global histogram path at this size"]}
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    m.close()
    g.close()


if __name__ == "__main__":
    main()
