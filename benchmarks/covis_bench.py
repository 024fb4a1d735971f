#!/usr/bin/env python3
"""The device covisibility graph on one MI355X (csrc/orbx_covis.hip).

    python benchmarks/covis_bench.py [--steps 3] [--warmup 1] [--repeats 5] [--loop-kf 1400]
                                     [--batches 1,256] [--out profiles/covis_bench.json]

Three measurements, each the median of `repeats` interleaved repeats (min and max beside it):
  (a) the observation refresh plus UpdateConnections of all keyframes in one batch on
      globalba_bench.py's synthetic loop map of --loop-kf keyframes (each call also alone);
  (b) UpdateConnections of one new keyframe (the last one) on that map, the other keyframes
      connected already;
  (c) assemble + LocalBundleAdjustment + apply at localba_bench.py's shape (12 + 20 keyframes,
      1500 points, about 9000 edges), B = 1 and B = 256 (the same local map in B disjoint copies
      of one map), beside LocalBundleAdjustment alone on the tables the assembly wrote, in the
      same session: the assembly's and the write-back's share of a LocalBA call.
The assembled problem's keyframe, point and edge counts are reported beside the scene's.  The
shapes are synthetic.  One JSON line, also written to --out.
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

LOOP_SHAPE = dict(window=6, pts_per_kf=8, n_loop=40, kind="mixed")
LOCAL_SHAPE = dict(n_free=12, n_fixed=20, n_pts=1500, kind="mixed", max_obs=8, outlier_frac=0.05, baseline=0.2)


def scene_map(sc):
    """mvpMapPoints of a local_ba_model scene: kf_mp [n_slots][cap] by keypoint row."""
    n_slots, cap = sc["kps_xy"].shape[:2]
    kf_mp = np.full((n_slots, cap), -1, np.int32)
    pt = np.repeat(np.arange(len(sc["pos"])), np.diff(sc["obs_off"]))
    kf_mp[np.asarray(sc["slot"])[sc["obs_kf"]], sc["obs_kp"]] = pt
    return kf_mp


def main(argv=None):
    ap = argparse.ArgumentParser(prog="covis_bench.py")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-kf", type=int, default=1400)
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "covis_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import global_ba_model as G
    import local_ba_model as M
    from orbslam2commentedbyxcm_amd import CovisibilityGraph
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster

    if not torch.cuda.is_available():
        raise SystemExit("covis_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lba = LocalBundleAdjuster()
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

    # ---- (a), (b): the loop map ----
    loop = G.make_banded(800, args.loop_kf, **LOOP_SHAPE)
    kf_mp = scene_map(loop)
    K, cap = kf_mp.shape
    n_mp = len(loop["pos"])
    g = CovisibilityGraph(K, cap, n_mp, max_conn=64)
    d_mp, d_n = t(kf_mp), t(np.full(K, cap, np.int32))
    d_bad, d_mpbad = torch.zeros(K, dtype=torch.uint8, device=dev), torch.zeros(n_mp, dtype=torch.uint8, device=dev)
    ids = np.arange(K, dtype=np.int32)
    last = np.array([args.loop_kf - 1], np.int32)

    def refresh():
        g.refresh_observations(d_mp, d_n, d_bad, d_mpbad, stream=stream)

    def refresh_and_all():
        refresh()
        g.update_connections(ids, stream=stream)

    res = {"loop_map": {"keyframes": int(args.loop_kf), "rows": K, "cap": cap, "mappoints": n_mp}}
    res["loop_map"].update(timed({"refresh": refresh, "update_all": lambda: g.update_connections(ids, stream=stream),
                                  "refresh_and_update_all": refresh_and_all,
                                  "update_one_new_keyframe": lambda: g.update_connections(last, stream=stream)}))
    torch.cuda.synchronize(dev)
    st = g.state()
    res["loop_map"]["observations"] = int(st["obs_off"][-1])
    res["loop_map"]["mean_connections"] = round(float(st["row_n"][:args.loop_kf].mean()), 2)
    res["loop_map"]["mean_list_length"] = round(float(st["ordered_n"][:args.loop_kf].mean()), 2)
    res["loop_map"]["status_or"] = int(np.bitwise_or.reduce(st["status"]))
    g.close()

    # ---- (c): localba_bench.py's shape, B disjoint copies in one map ----
    sc = M.make_scene(900, **LOCAL_SHAPE)
    one = scene_map(sc)
    S, cap = one.shape
    P = len(sc["pos"])
    n_kf, n_obs = len(sc["fixed"]), len(sc["obs_kf"])
    free = np.flatnonzero(np.asarray(sc["fixed"]) == 0)
    kps1 = np.zeros((S, cap), L.KEYPOINT_DTYPE)
    kps1["x"], kps1["y"], kps1["octave"] = sc["kps_xy"][..., 0], sc["kps_xy"][..., 1], sc["kps_oct"]
    pose1 = np.zeros((S, 12), np.float32)
    pose1[np.asarray(sc["slot"])] = np.asarray(sc["Tcw"], np.float32).reshape(-1, 12)
    fx, fy, cx, cy, bf = sc["cam"]
    # the walk leaves out the points that only fixed cameras see: the assembled problem is a little
    # smaller than the scene (counts_problem0 = keyframe rows, point rows, edges)
    res["local_map"] = {"shape": LOCAL_SHAPE, "scene_counts": [n_kf, P, n_obs]}
    for B in [int(b) for b in args.batches.split(",")]:
        kf_mp = np.concatenate([np.where(one >= 0, one + b * P, -1) for b in range(B)]).astype(np.int32)
        g = CovisibilityGraph(S * B, cap, P * B, max_conn=64)
        d_mp = t(kf_mp)
        d_n_full = t(np.full(S * B, cap, np.int32))
        # the free keyframes connect among themselves while the others' rows are empty, as if the
        # fixed cameras shared fewer than 15 points with them; then every row is observed
        n_free_only = np.zeros(S * B, np.int32)
        free_ids = np.concatenate([np.asarray(sc["slot"])[free] + b * S for b in range(B)]).astype(np.int32)
        n_free_only[free_ids] = cap
        g.refresh_observations(d_mp, t(n_free_only), None, None, n_mappoints=P * B, stream=stream)
        g.update_connections(free_ids, stream=stream)
        g.refresh_observations(d_mp, d_n_full, None, None, n_mappoints=P * B, stream=stream)
        cur = (int(np.asarray(sc["slot"])[free[0]]) + S * np.arange(B)).astype(np.int32)
        d_pose = t(np.tile(pose1, (B, 1)))
        d_pos = t(np.tile(np.asarray(sc["pos"], np.float32).reshape(-1, 3), (B, 1)))
        d_pose0, d_pos0, d_mp0 = d_pose.clone(), d_pos.clone(), d_mp.clone()
        d_kps = t(np.tile(kps1, (B, 1)).view(np.uint8).reshape(S * B, cap * 28)).view(S * B, cap, 28)
        d_ur = t(np.tile(np.asarray(sc["u_right"], np.float32), (B, 1)))
        caps = (n_kf * B + 8, P * B + 8, n_obs * B + 8)
        tab = lba.assemble_batch_device(g, cur, d_pose, d_pos, *caps, stream=stream)
        out = lba.local_ba_assembled_device(tab, d_kps, d_ur, sc["inv_sigma2"], fx, fy, cx, cy, bf, max_free_kf=16,
                                            stream=stream)
        torch.cuda.synchronize(dev)
        counts = tab["counts"].cpu().numpy()

        def assemble():
            lba.assemble_batch_device(g, cur, d_pose, d_pos, *caps, tables=tab, stream=stream)

        def local_ba():
            lba.local_ba_assembled_device(tab, d_kps, d_ur, sc["inv_sigma2"], fx, fy, cx, cy, bf, out=out, max_free_kf=16,
                                          stream=stream)

        def apply():
            lba.apply_batch_device(g, tab, out["kf_Tcw_opt"], out["pt_pos_opt"], out["erase"], d_pose, d_pos, d_mp,
                                   stream=stream)

        def chain():
            d_pose.copy_(d_pose0)
            d_pos.copy_(d_pos0)
            d_mp.copy_(d_mp0)
            assemble()
            local_ba()
            apply()

        r = timed({"assemble": assemble, "local_ba_alone": local_ba, "apply": apply, "assemble_local_ba_apply": chain})
        la = r["local_ba_alone"]["ms_per_call"]
        r.update({"batch": B, "counts_problem0": counts[0].tolist(),
                  "every_problem_has_these_counts": bool((counts == counts[0]).all()),
                  "assembly_status_or": int(np.bitwise_or.reduce(tab["status"].cpu().numpy())),
                  "local_ba_status_or": int(np.bitwise_or.reduce(out["status"].cpu().numpy())),
                  "mean_erased": float(out["n_erase"].cpu().numpy().mean()),
                  "assemble_share_of_local_ba": round(r["assemble"]["ms_per_call"] / la, 4),
                  "apply_share_of_local_ba": round(r["apply"]["ms_per_call"] / la, 4)})
        res["local_map"][f"b{B}"] = r
        g.close()

    a = res["loop_map"]
    out = {"metric": f"keyframes/s observation refresh + UpdateConnections of all, {args.loop_kf}-keyframe loop map",
           "value": round(args.loop_kf / (a["refresh_and_update_all"]["ms_per_call"] * 1e-3), 1), "unit": "keyframes/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True,
           "dtype": "i32", "data": "synthetic", **res,
           "not_measured": ["a real sequence's map (the shapes are synthetic)", "maps past --loop-kf keyframes",
                            "the split of k_covis_assemble between its passes"]}
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    lba.close()


if __name__ == "__main__":
    main()
