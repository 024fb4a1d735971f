#!/usr/bin/env python3
"""Device LocalBundleAdjustment on one MI355X (orbx_local_bundle_adjustment_batch_device,
csrc/orbx_localba.hip).

    python benchmarks/localba_bench.py [--batches 1,64,256] [--steps 3] [--warmup 1] [--repeats 5]
                                       [--single-calls 12] [--out profiles/localba_bench.json]

A local-map shape built from tests/local_ba_model.py's scene maker: 12 free + 20 fixed
keyframes, 1500 points, about 9000 edges, a third of them monocular, 1 px x scale noise, 5 %
gross outliers (these figures are a typical ORB-SLAM2 local map by reading, not measured).  8
different maps are repeated over the batch; they share their keypoint rows.  The batch sizes are
measured interleaved, `repeats` times each; the median is reported with min and max.  The
first problems are compared with the model (flags, count, trace; the bench scenes are not
guarded, so a difference is reported, not asserted).  One JSON line, also written to --out.
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

SHAPE = dict(n_free=12, n_fixed=20, n_pts=1500, kind="mixed", max_obs=8, outlier_frac=0.05, baseline=0.2)
MAX_FREE = 16


def main(argv=None):
    ap = argparse.ArgumentParser(prog="localba_bench.py")
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=12)
    ap.add_argument("--parity", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "localba_bench.json"))
    args = ap.parse_args(argv)
    batches = [int(b) for b in args.batches.split(",")]

    import torch

    import local_ba_model as M
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster

    if not torch.cuda.is_available():
        raise SystemExit("localba_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    opt = LocalBundleAdjuster()
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    scenes = [M.make_scene(900 + s, **SHAPE) for s in range(8)]
    A = M.batch_arrays(scenes)
    kps = np.zeros(A["kps_xy"].shape[:2], L.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = A["kps_xy"][..., 0], A["kps_xy"][..., 1], A["kps_oct"]
    d_kps = t(kps.view(np.uint8).reshape(A["n_slots"], A["cap"] * 28)).view(A["n_slots"], A["cap"], 28)
    d_ur = t(A["u_right"])
    s0 = scenes[0]
    fx, fy, cx, cy, bf = s0["cam"]

    def tables(B):
        """B problems: the 8 maps in turn, their keypoint rows shared."""
        kf_off, pt_off, obs_off = [0], [0], [0]
        rows = {k: [] for k in ("Tcw", "fixed", "slot", "pos", "obs_kf", "obs_kp")}
        for b in range(B):
            s = b % 8
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
        n_kf, n_pt, n_obs = kf_off[-1], pt_off[-1], obs_off[-1]
        d["T"] = torch.zeros((n_kf, 12), dtype=torch.float32, device=dev)
        d["X"] = torch.zeros((n_pt, 3), dtype=torch.float32, device=dev)
        d["erase"] = torch.zeros((n_obs,), dtype=torch.uint8, device=dev)
        d["level1"] = torch.zeros((n_obs,), dtype=torch.uint8, device=dev)
        d["n_erase"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        d["status"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        d["trace"] = torch.zeros((B, 2, 2), dtype=torch.int32, device=dev)
        d["edges"] = n_obs / B
        return d

    data = {B: tables(B) for B in batches}

    def step(B):
        d = data[B]
        opt.local_ba_batch_device(d["kf_off"], d["Tcw"], d["fixed"], d["slot"], d["pt_off"], d["pos"], d["obs_off"],
                                  d["obs_kf"], d["obs_kp"], d_kps, d_ur, s0["inv_sigma2"], fx, fy, cx, cy, bf, d["T"],
                                  d["X"], d["erase"], d["n_erase"], d["status"], d_level1=d["level1"], d_trace=d["trace"],
                                  max_free_kf=MAX_FREE, stream=stream)

    for B in batches:
        for _ in range(max(1, args.warmup)):
            step(B)
    torch.cuda.synchronize(dev)
    times = {B: [] for B in batches}
    for _ in range(args.repeats):
        for B in batches:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(B)
            torch.cuda.synchronize(dev)
            times[B].append((time.perf_counter() - t0) / args.steps)

    res_b = {}
    for B in batches:
        d = data[B]
        ms = sorted(1e3 * x for x in times[B])
        med = statistics.median(ms)
        tr = d["trace"].cpu().numpy()
        res_b[str(B)] = {"edges_per_problem": round(d["edges"], 1), "ms_per_call": round(med, 3), "ms_min": round(ms[0], 3),
                         "ms_max": round(ms[-1], 3), "us_per_problem": round(1e3 * med / B, 1),
                         "problems_per_s": round(B / (med * 1e-3), 1),
                         "mean_lm_iterations": float(tr[:, :, 0].sum(axis=1).mean()),
                         "mean_linear_solves": float(tr[:, :, 1].sum(axis=1).mean()),
                         "mean_erased": float(d["n_erase"].cpu().numpy().mean()),
                         "status_or": int(np.bitwise_or.reduce(d["status"].cpu().numpy()))}

    # parity of the first problems with the model
    B0 = batches[-1]
    d = data[B0]
    got = {k: d[k].cpu().numpy() for k in ("erase", "level1", "n_erase", "trace", "T", "X", "obs_off", "pt_off", "kf_off")}
    checked, same, dT, dX = min(args.parity, B0, 8), 0, 0.0, 0.0
    for b in range(checked):
        r = M.local_ba(scenes[b])
        p0, p1 = got["pt_off"][b:b + 2]
        k0, k1 = got["kf_off"][b:b + 2]
        o0, o1 = got["obs_off"][p0], got["obs_off"][p1]
        same += int(np.array_equal(got["erase"][o0:o1], r["erase"]) and np.array_equal(got["level1"][o0:o1], r["level1"])
                    and got["n_erase"][b] == r["n_erase"] and np.array_equal(got["trace"][b], r["trace"]))
        dT = max(dT, float(np.abs(got["T"][k0:k1].astype(np.float64) - r["Tcw"]).max()))
        dX = max(dX, float(np.abs(got["X"][p0:p1].astype(np.float64) - r["pos"]).max()))

    keys1 = np.zeros(s0["kps_xy"].shape[:2], L.KEYPOINT_DTYPE)
    keys1["x"], keys1["y"], keys1["octave"] = s0["kps_xy"][..., 0], s0["kps_xy"][..., 1], s0["kps_oct"]
    us = []
    for _ in range(args.single_calls):
        opt.LocalBundleAdjustment(s0["Tcw"], s0["fixed"], s0["slot"], s0["pos"], s0["obs_off"], s0["obs_kf"], s0["obs_kp"],
                                  keys1, s0["u_right"], s0["inv_sigma2"], fx, fy, cx, cy, bf, max_free_kf=MAX_FREE)
        us.append(opt.last_call_us())
    us = sorted(us[2:])
    top = res_b[str(B0)]
    res = {"metric": f"local maps/s LocalBundleAdjustment, batch {B0}, 12 + 20 keyframes, 1500 points",
           "value": top["problems_per_s"], "unit": "problems/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "higher_is_better": True, "dtype": "f64", "data": "synthetic", "shape": SHAPE,
           "max_free_kf": MAX_FREE, "batches": res_b,
           "host_form_b1_us": {"median": round(statistics.median(us), 1), "min": round(us[0], 1), "max": round(us[-1], 1)},
           "parity": {"problems_checked": checked, "identical_flags_count_trace": same, "max_pose_entry_diff": dT,
                      "max_position_entry_diff": dX},
           "kernels": {"k_local_ba": {"threads": 256, "vgprs": 253, "agprs": 0, "sgprs": 106, "scratch_bytes": 24,
                                      "lds_bytes": 21944, "waves_per_simd": 2}}}
    line = json.dumps(res)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    opt.close()


if __name__ == "__main__":
    main()
