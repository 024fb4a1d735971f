#!/usr/bin/env python3
"""Device PnPsolver throughput on one MI355X (orbx_pnp_*, csrc/orbx_pnp.hip).

    python benchmarks/pnp_bench.py [--batch 256] [--steps 10] [--warmup 2] [--repeats 5]
                                   [--out profiles/pnp_bench.json]

B = --batch relocalisation candidates (lost frames x candidate keyframes), built like
tests/pnp_scenes.py's scenes (TUM1, 0.5 px noise, 20 % gross outliers, Tracking::Relocalization's
parameters 0.99, 10, 300, 4, 0.5, 5.991): 100 matches among 1000 keypoints in rows of cap 1024,
16 distinct candidates tiled.  Two schedules, each including the set (the constructor and
SetRansacParameters):
  rounds the reference's (Tracking.cc:1570-1680): iterate(5) on the whole batch, the host reads
         found / no_more back after every round, until every candidate has returned a pose or
         has no more;
  find   one call that runs to the iteration cap.
The repeats of the two are interleaved; each repeat times --steps schedules between two
synchronisations.  Reported: the median over repeats with min / max (ms per batch, us per
candidate, candidates/s), the single host call's latency inside the library (one iterate(5)),
and parity of the first candidates with the model.

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

CAP, SLOTS, MATCHES, ROUND = 1024, 1000, 100, 5
OUT_I32 = ("found", "no_more", "n_inliers", "refined", "best_inliers", "best_iteration", "iterations", "n_corr",
           "min_inliers_used", "max_its_used", "status")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="pnp_bench.py")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pnp_bench.json"))
    args = ap.parse_args(argv)
    B = args.batch

    import torch

    import pnp_scenes as S
    from orbslam2commentedbyxcm_amd.pnp import PnPsolver

    if not torch.cuda.is_available():
        raise SystemExit("pnp_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    scenes = [S.build(dict(seed=900 + k, N=MATCHES, n=SLOTS, out=0.2, noise=0.5, blind=False), f"bench_{k}")
              for k in range(16)]
    P = S.pack([scenes[b % 16] for b in range(B)], cap=CAP)
    p = P["params"]
    solver = PnPsolver(max_batch=B, cap=CAP, max_draws=S.N_DRAWS)
    stream = torch.cuda.Stream(dev)   # the library's kernels and torch's flag arithmetic in one order
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = dict(kps=t(P["kps"].view(np.uint8).reshape(B, CAP, 28)), n=t(P["n"]), matches=t(P["matches"]), pos=t(P["pos"]),
             draws=t(P["draws"]))
    o = {k: torch.zeros((B,), dtype=torch.int32, device=dev) for k in OUT_I32}
    o["inliers"] = torch.zeros((B, CAP), dtype=torch.uint8, device=dev)
    o["frame_mp"] = torch.zeros((B, CAP), dtype=torch.int32, device=dev)
    o["Tcw"] = torch.zeros((B, 12), dtype=torch.float32, device=dev)
    done = torch.zeros((B,), dtype=torch.int32, device=dev)

    def set_batch():
        solver.set_batch_device(d["kps"], d["n"], d["matches"], d["pos"], S.SIGMA2, S.K, d["draws"],
                                probability=p["probability"], min_inliers=p["min_inliers"],
                                max_iterations=p["max_iterations"], min_set=p["min_set"], epsilon=p["epsilon"],
                                th2=p["th2"], stream=stream)

    def run_find():
        set_batch()
        solver.iterate_batch_device(0, stream=stream, **o)   # a first call runs to the cap (cc:226)
        return 1

    def run_rounds():
        set_batch()
        done.zero_()
        rounds = 0
        while True:
            solver.iterate_batch_device(ROUND, stream=stream, **o)
            rounds += 1
            done.__ior__(o["found"] | o["no_more"])
            if bool(done.all().item()):   # the read-back the reference's loop makes per round
                return rounds

    runs = {"rounds": run_rounds, "find": run_find}
    nrounds = 0
    for sched in runs:
        for _ in range(max(1, args.warmup)):
            r = runs[sched]()
            if sched == "rounds":
                nrounds = r
    torch.cuda.synchronize(dev)
    times = {c: [] for c in runs}
    for _ in range(args.repeats):
        for c in runs:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                runs[c]()
            torch.cuda.synchronize(dev)
            times[c].append((time.perf_counter() - t0) / args.steps)

    # parity of the first candidates with the model after find() (the bench scenes are not
    # guarded: a difference is reported, not asserted)
    run_find()
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in o.items()}
    checked, same = min(4, B), 0
    for b in range(checked):
        sc = scenes[b % 16]
        r = S.model_for(sc).iterate(0)
        same += int(all(int(got[k][b]) == int(r[k]) for k in OUT_I32)
                    and np.array_equal(got["inliers"][b, :sc["n"]], r["inliers"]))
    sc = scenes[0]
    one = PnPsolver(sc["keys"], sc["matches"], sc["pos"], S.SIGMA2, S.K, draws=sc["draws"])
    us = []
    for _ in range(args.single_calls):
        one.SetRansacParameters(p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"],
                                p["th2"])
        one.iterate_host(ROUND)
        us.append(one.last_call_us())
    one.close()
    us = sorted(us[3:])
    res = {"metric": f"candidates/s PnPsolver, batch {B}, iterate(5) rounds", "unit": "candidates/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True,
           "dtype": "f64", "data": "synthetic", "batch": B, "keypoints": SLOTS, "matches": MATCHES, "cap": CAP,
           "returned": int(got["found"].sum()), "refined": int(got["refined"].sum()),
           "mean_iterations_to_stop": float(got["iterations"].mean()), "rounds_of_5": nrounds,
           "single_iterate5_us": {"median": round(statistics.median(us), 1), "min": round(us[0], 1),
                                  "max": round(us[-1], 1)},
           "parity": {"candidates_checked": checked, "identical": same}}
    for sched in runs:
        ms = sorted(1e3 * x for x in times[sched])
        med = statistics.median(ms)
        res[sched] = {"ms_per_batch": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                      "us_per_candidate": round(1e3 * med / B, 3), "candidates_per_s": round(B / (med * 1e-3), 1)}
    res["value"] = res["rounds"]["candidates_per_s"]
    line = json.dumps(res)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    solver.close()


if __name__ == "__main__":
    main()
