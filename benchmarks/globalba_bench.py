#!/usr/bin/env python3
"""Device BundleAdjustment / GlobalBundleAdjustemnt on one MI355X
(orbx_global_bundle_adjustment_batch_device, csrc/orbx_globalba.hip).

    python benchmarks/globalba_bench.py [--steps 3] [--warmup 1] [--repeats 5] [--loop-kf 1400]
                                        [--out profiles/globalba_bench.json]

Three measurements, each the median of `repeats` interleaved repeats (min and max beside it):
  (a) initial maps as Tracking::CreateInitialMapMonocular hands them over: 1 fixed + 1 free
      keyframe, 300 monocular points, 20 iterations, robust; 8 different maps repeated over the
      batch, at B = 1 and B = 256;
  (b) one loop-closure map as LoopClosing::RunGlobalBundleAdjustment hands it over: a trajectory
      of --loop-kf keyframes out and back, every point seen by a window of consecutive keyframes,
      loop points between both ends, 10 iterations, not robust; B = 1 and B = 4 (the same map);
  (c) the yardstick: benchmarks/localba_bench.py's own local-map shape through k_local_ba (its two
      optimisations) and through k_global_ba (5 iterations, robust), as time per LM trial.
For each: the envelope blocks, LM iterations, solves, status, chi2 before and after, and whether
two runs give the same bytes.  The first problems of (a) are compared with the model (the bench
scenes are not guarded, so a difference is reported, not asserted).  The shapes are typical by
reading, not measured on a sequence.  One JSON line, also written to --out.
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

INIT_SHAPE = dict(n_free=1, n_fixed=1, n_pts=300, kind="mono")
LOOP_SHAPE = dict(window=6, pts_per_kf=8, n_loop=40, kind="mixed")
LOCAL_SHAPE = dict(n_free=12, n_fixed=20, n_pts=1500, kind="mixed", max_obs=8, outlier_frac=0.05, baseline=0.2)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="globalba_bench.py")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-kf", type=int, default=1400)
    ap.add_argument("--parity", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "globalba_bench.json"))
    args = ap.parse_args(argv)

    import torch

    import global_ba_model as G
    import local_ba_model as M
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.optimizer import GlobalBundleAdjuster, LocalBundleAdjuster, global_ba_envelope

    if not torch.cuda.is_available():
        raise SystemExit("globalba_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    opt = GlobalBundleAdjuster()
    lba = LocalBundleAdjuster(matcher=opt)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def problem_set(scenes, B):
        """B problems: the scenes in turn, their keypoint rows shared."""
        A = M.batch_arrays(scenes)
        kps = np.zeros(A["kps_xy"].shape[:2], L.KEYPOINT_DTYPE)
        kps["x"], kps["y"], kps["octave"] = A["kps_xy"][..., 0], A["kps_xy"][..., 1], A["kps_oct"]
        kf_off, pt_off, obs_off = [0], [0], [0]
        rows = {k: [] for k in ("Tcw", "fixed", "slot", "pos", "obs_kf", "obs_kp")}
        for b in range(B):
            s = b % len(scenes)
            k0, k1 = A["kf_off"][s:s + 2]
            p0, p1 = A["pt_off"][s:s + 2]
            o0, o1 = A["obs_off"][p0], A["obs_off"][p1]
            for k, (a, c) in (("Tcw", (k0, k1)), ("fixed", (k0, k1)), ("slot", (k0, k1)), ("pos", (p0, p1)),
                              ("obs_kf", (o0, o1)), ("obs_kp", (o0, o1))):
                rows[k].append(A[k][a:c])
            obs_off.extend((A["obs_off"][p0 + 1:p1 + 1] - o0 + obs_off[-1]).tolist())
            kf_off.append(kf_off[-1] + k1 - k0)
            pt_off.append(pt_off[-1] + p1 - p0)
        d = {k: t(np.concatenate(v)) for k, v in rows.items()}
        d["kf_off"], d["pt_off"], d["obs_off"] = (t(np.asarray(v, np.int32)) for v in (kf_off, pt_off, obs_off))
        d["kps"] = t(kps.view(np.uint8).reshape(A["n_slots"], A["cap"] * 28)).view(A["n_slots"], A["cap"], 28)
        d["ur"] = t(A["u_right"])
        n_kf, n_pt, n_obs = kf_off[-1], pt_off[-1], obs_off[-1]
        d["T"] = torch.zeros((n_kf, 12), dtype=torch.float32, device=dev)
        d["X"] = torch.zeros((n_pt, 3), dtype=torch.float32, device=dev)
        d["inc"] = torch.zeros((n_pt,), dtype=torch.uint8, device=dev)
        d["status"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        d["trace"] = torch.zeros((B, 2), dtype=torch.int32, device=dev)
        d["chi2"] = torch.zeros((B, 2), dtype=torch.float64, device=dev)
        d["erase"] = torch.zeros((n_obs,), dtype=torch.uint8, device=dev)
        d["n_erase"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        d["ltrace"] = torch.zeros((B, 2, 2), dtype=torch.int32, device=dev)
        d["B"], d["edges"], d["kf"], d["pts"] = B, n_obs / B, n_kf / B, n_pt / B
        d["blocks"] = max(global_ba_envelope(s["fixed"], s["obs_off"], s["obs_kf"]) for s in scenes)
        d["cam"], d["sig"] = scenes[0]["cam"], scenes[0]["inv_sigma2"]
        d["free"] = int((np.asarray(scenes[0]["fixed"]) == 0).sum())
        return d

    def gba(d, iterations, robust):
        fx, fy, cx, cy, bf = d["cam"]
        opt.global_ba_batch_device(d["kf_off"], d["Tcw"], d["fixed"], d["slot"], d["pt_off"], d["pos"], d["obs_off"],
                                   d["obs_kf"], d["obs_kp"], d["kps"], d["ur"], d["sig"], fx, fy, cx, cy, bf, iterations,
                                   robust, d["blocks"], d["T"], d["X"], d["inc"], d["status"], d_trace=d["trace"],
                                   d_chi2=d["chi2"], stream=stream)

    def local(d):
        fx, fy, cx, cy, bf = d["cam"]
        lba.local_ba_batch_device(d["kf_off"], d["Tcw"], d["fixed"], d["slot"], d["pt_off"], d["pos"], d["obs_off"],
                                  d["obs_kf"], d["obs_kp"], d["kps"], d["ur"], d["sig"], fx, fy, cx, cy, bf, d["T"], d["X"],
                                  d["erase"], d["n_erase"], d["status"], d_trace=d["ltrace"], max_free_kf=16, stream=stream)

    t0 = time.perf_counter()
    init_scenes = [M.make_scene(700 + s, **INIT_SHAPE) for s in range(8)]
    loop_scene = G.make_banded(800, args.loop_kf, **LOOP_SHAPE)
    local_scenes = [M.make_scene(900 + s, **LOCAL_SHAPE) for s in range(8)]
    t_scenes = time.perf_counter() - t0
    runs = {
        "init_b1": (problem_set(init_scenes, 1), lambda d: gba(d, 20, True)),
        "init_b256": (problem_set(init_scenes, 256), lambda d: gba(d, 20, True)),
        "loop_b1": (problem_set([loop_scene], 1), lambda d: gba(d, 10, False)),
        "loop_b4": (problem_set([loop_scene], 4), lambda d: gba(d, 10, False)),
        "local_shape_k_global_ba_b1": (problem_set(local_scenes, 1), lambda d: gba(d, 5, True)),
        "local_shape_k_global_ba_b64": (problem_set(local_scenes, 64), lambda d: gba(d, 5, True)),
        "local_shape_k_local_ba_b1": (problem_set(local_scenes, 1), local),
        "local_shape_k_local_ba_b64": (problem_set(local_scenes, 64), local),
    }

    same = {}
    for name, (d, fn) in runs.items():                       # warm-up, and two runs' bytes
        for _ in range(max(1, args.warmup)):
            fn(d)
        torch.cuda.synchronize(dev)
        first = [d[k].cpu().numpy().tobytes() for k in ("T", "X", "status")]
        fn(d)
        torch.cuda.synchronize(dev)
        same[name] = first == [d[k].cpu().numpy().tobytes() for k in ("T", "X", "status")]
    times = {name: [] for name in runs}
    for _ in range(args.repeats):
        for name, (d, fn) in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn(d)
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) / args.steps)

    res = {}
    for name, (d, fn) in runs.items():
        ms = sorted(1e3 * x for x in times[name])
        med = statistics.median(ms)
        is_local = fn is local
        tr = d["ltrace"].cpu().numpy().sum(axis=1) if is_local else d["trace"].cpu().numpy()
        r = {"batch": d["B"], "keyframes": d["kf"], "points": d["pts"], "edges_per_problem": round(d["edges"], 1),
             "ms_per_call": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
             "us_per_problem": round(1e3 * med / d["B"], 1), "mean_lm_iterations": float(tr[:, 0].mean()),
             "mean_linear_solves": float(tr[:, 1].mean()),
             "us_per_problem_per_solve": round(1e3 * med / d["B"] / max(float(tr[:, 1].mean()), 1.0), 1),
             "status_or": int(np.bitwise_or.reduce(d["status"].cpu().numpy())), "two_runs_same_bytes": bool(same[name])}
        if not is_local:
            c = d["chi2"].cpu().numpy()
            r.update({"envelope_blocks": int(d["blocks"]), "dense_blocks": d["free"] * (d["free"] + 1) // 2,
                      "chi2_initial_problem0": float(c[0, 0]), "chi2_final_problem0": float(c[0, 1])})
        res[name] = r

    # parity of (a)'s first problems with the model
    d = runs["init_b256"][0]
    got = {k: d[k].cpu().numpy() for k in ("T", "X", "trace", "inc")}
    checked, ok, dT, dX = min(args.parity, 8), 0, 0.0, 0.0
    for b in range(checked):
        r = G.global_ba(init_scenes[b], iterations=20, robust=True)
        ok += int(np.array_equal(got["trace"][b], r["trace"]) and np.array_equal(got["inc"][300 * b:300 * b + 300], r["pt_included"]))
        dT = max(dT, float(np.abs(got["T"][2 * b:2 * b + 2].astype(np.float64) - r["Tcw"]).max()))
        dX = max(dX, float(np.abs(got["X"][300 * b:300 * b + 300].astype(np.float64) - r["pos"]).max()))

    ratio = {b: round(res[f"local_shape_k_global_ba_{b}"]["us_per_problem_per_solve"]
                      / res[f"local_shape_k_local_ba_{b}"]["us_per_problem_per_solve"], 3) for b in ("b1", "b64")}
    out = {"metric": "initial maps/s BundleAdjustment, batch 256, 1 + 1 keyframes, 300 monocular points, 20 iterations",
           "value": round(256 / (res["init_b256"]["ms_per_call"] * 1e-3), 1), "unit": "problems/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "f64",
           "data": "synthetic", "shapes": {"init": INIT_SHAPE, "loop": dict(LOOP_SHAPE, n_kf=args.loop_kf),
                                           "local": LOCAL_SHAPE}, "scene_build_s": round(t_scenes, 1), "runs": res,
           "k_global_ba_over_k_local_ba_per_trial": ratio,
           "parity_init": {"problems_checked": checked, "identical_trace_and_flags": ok, "max_pose_entry_diff": dT,
                           "max_position_entry_diff": dX},
           "kernels": {"k_global_ba": {"threads": 256, "vgprs": 226, "agprs": 0, "sgprs": 106, "scratch_bytes": 24,
                                       "lds_bytes": 96, "waves_per_simd": 2}},
           "not_measured": ["a real sequence's maps (the shapes are synthetic)", "maps past --loop-kf keyframes",
                            "the host form's staging time for the loop map", "the split of a call between "
                            "linearisation, Schur complement and factorisation"]}
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    opt.close()


if __name__ == "__main__":
    main()
