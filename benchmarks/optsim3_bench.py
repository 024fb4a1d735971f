#!/usr/bin/env python3
"""Device OptimizeSim3 throughput on one MI355X (orbx_optimize_sim3_batch_device,
csrc/orbx_optsim3.hip).

    python benchmarks/optsim3_bench.py [--batch 256] [--steps 10] [--warmup 2] [--repeats 5]
                                       [--sim3-json profiles/sim3_bench.json]
                                       [--out profiles/optsim3_bench.json]

B = --batch loop candidates at sim3_bench.py's loop shape: about 150 pairs among 2000 slots
(cap 2048), built from tests/optimize_sim3_model.py's scenes (TUM1, points 1.5-8 m away, 1 px x
scale noise, 30 % gross outliers, a start 2 deg / 5 cm / 3 % off, th2 = 10), 16 distinct
candidates tiled, with fix_scale 0 and 1.  matches12 is in/out, so every step first restores it
with a device copy; that copy is inside the timed region.  The two settings' repeats are
interleaved; each repeat times --steps calls between two synchronisations.  Reported: the
median over repeats with min / max (ms per batch, us per candidate, candidates/s), the single
host call's latency inside the library, and parity of the first candidates with the model.
--sim3-json: a sim3_bench.py result measured on the same box; its find() figure at the loop
shape is recorded beside these.

Prints ONE JSON line and writes it to --out.  No rate has been measured for this stage by
anyone, so no target is set: the file is the record.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "tests", ROOT / "benchmarks"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

SHAPE = dict(npairs=150, nout=45, cap1=2048, n_slots=2000)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="optsim3_bench.py")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=30)
    ap.add_argument("--sim3-json", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "optsim3_bench.json"))
    args = ap.parse_args(argv)
    B = args.batch

    import torch

    import optimize_sim3_model as M
    from orbslam2commentedbyxcm_amd.optimizer import Sim3Optimizer

    if not torch.cuda.is_available():
        raise SystemExit("optsim3_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    opt = Sim3Optimizer()
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    data = {}
    for fix in (False, True):
        scenes = [M.make_scene(700 + s, fix_scale=fix, **SHAPE) for s in range(16)]
        P = M.pack([scenes[b % 16] for b in range(B)])
        cap1, cap2 = P["cap1"], P["cap2"]
        d = {k: t(P[k]) for k in ("n1", "mp1", "idx2", "n2", "pos", "Tcw1", "Tcw2", "R12", "t12", "s12")}
        d["kps1"] = t(P["kps1"].view(np.uint8).reshape(B, cap1 * 28))
        d["kps2"] = t(P["kps2"].view(np.uint8).reshape(B, cap2 * 28))
        d["m12_in"], d["m12"] = t(P["m12"]), t(P["m12"])
        d["R"] = torch.zeros((B, 9), dtype=torch.float32, device=dev)
        d["t"] = torch.zeros((B, 3), dtype=torch.float32, device=dev)
        d["s"] = torch.zeros((B,), dtype=torch.float32, device=dev)
        for k in ("ninliers", "ncorr", "nbad"):
            d[k] = torch.zeros((B,), dtype=torch.int32, device=dev)
        d["trace"] = torch.zeros((B, 2, 2), dtype=torch.int32, device=dev)
        data[fix] = (scenes, d)

    def step(fix):
        sc, d = data[fix]
        s0 = sc[0]
        d["m12"].copy_(d["m12_in"])
        opt.optimize_sim3_batch_device(d["kps1"], d["n1"], d["mp1"], d["m12"], d["idx2"], d["kps2"], d["n2"], d["pos"],
                                       d["Tcw1"], d["Tcw2"], s0["inv_sigma2_1"], s0["inv_sigma2_2"], s0["K1"], s0["K2"],
                                       d["R12"], d["t12"], d["s12"], float(s0["th2"]), fix, d["R"], d["t"], d["s"],
                                       d_ninliers=d["ninliers"], d_ncorr=d["ncorr"], d_nbad=d["nbad"],
                                       d_trace=d["trace"], stream=stream)

    for fix in data:
        for _ in range(max(1, args.warmup)):
            step(fix)
    torch.cuda.synchronize(dev)
    times = {fix: [] for fix in data}
    for _ in range(args.repeats):
        for fix in data:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(fix)
            torch.cuda.synchronize(dev)
            times[fix].append((time.perf_counter() - t0) / args.steps)

    res_w = {}
    for fix, (sc, d) in data.items():
        step(fix)
        torch.cuda.synchronize(dev)
        got = {k: d[k].cpu().numpy() for k in ("ninliers", "ncorr", "nbad", "trace")}
        checked, same = min(4, B), 0
        for b in range(checked):   # the bench scenes are not guarded: a difference is reported, not asserted
            r = M.optimize_sim3(sc[b % 16])
            same += int(got["ninliers"][b] == r["ninliers"] and got["nbad"][b] == r["nbad"]
                        and got["ncorr"][b] == r["ncorr"] and np.array_equal(got["trace"][b], r["trace"]))
        s0 = sc[0]
        n1, n2 = s0["n1"], s0["n2"]
        us = []
        for _ in range(args.single_calls):
            opt.OptimizeSim3(M.keypoints(s0["k1_xy"][:n1], s0["k1_oct"][:n1]), s0["mp1"][:n1], s0["matches12"][:n1],
                             s0["idx2"][:n1], M.keypoints(s0["k2_xy"][:n2], s0["k2_oct"][:n2]), s0["mp_pos"],
                             s0["Tcw1"], s0["Tcw2"], s0["inv_sigma2_1"], s0["inv_sigma2_2"], s0["K1"], s0["K2"],
                             s0["R12"], s0["t12"], s0["s12"], s0["th2"], fix)
            us.append(opt.last_call_us())
        us = sorted(us[3:])
        ms = sorted(1e3 * x for x in times[fix])
        med = statistics.median(ms)
        res_w["fix_scale" if fix else "free_scale"] = {
            "pairs": int(got["ncorr"].mean()), "slots": SHAPE["n_slots"], "cap": SHAPE["cap1"],
            "mean_rejected_first_pass": float(got["nbad"].mean()), "mean_inliers": float(got["ninliers"].mean()),
            "mean_lm_iterations": float(got["trace"][:, :, 0].sum(axis=1).mean()),
            "mean_linear_solves": float(got["trace"][:, :, 1].sum(axis=1).mean()),
            "ms_per_batch": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
            "us_per_candidate": round(1e3 * med / B, 3), "candidates_per_s": round(B / (med * 1e-3), 1),
            "single_call_us": {"median": round(statistics.median(us), 1), "min": round(us[0], 1),
                               "max": round(us[-1], 1)},
            "parity": {"candidates_checked": checked, "identical": same}}

    sim3 = None
    if args.sim3_json:
        j = json.loads(Path(args.sim3_json).read_text())
        sim3 = {"batch": j["batch"], "find_ms_per_batch": j["workloads"]["loop"]["find"]["ms_per_batch"],
                "rounds_ms_per_batch": j["workloads"]["loop"]["rounds"]["ms_per_batch"]}
    res = {"metric": f"candidates/s OptimizeSim3, batch {B}, free scale, loop density",
           "value": res_w["free_scale"]["candidates_per_s"], "unit": "candidates/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "f64",
           "data": "synthetic", "batch": B, "workloads": res_w, "sim3_solver_same_box_loop_shape": sim3,
           "kernels": {"k_opt_sim3": {"threads": 256, "vgprs": 256, "agprs": 54, "sgprs": 106, "scratch_bytes": 0,
                                      "lds_bytes": 32064, "waves_per_simd": 1}}}
    line = json.dumps(res)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    opt.close()


if __name__ == "__main__":
    main()
