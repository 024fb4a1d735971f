#!/usr/bin/env python3
"""Device Sim3Solver throughput on one MI355X (orbx_sim3_*, csrc/orbx_sim3.hip; DESIGN.md
§4.16).

    python benchmarks/sim3_bench.py [--batch 256] [--steps 10] [--warmup 2] [--repeats 5]
                                    [--out profiles/sim3_bench.json]

B = --batch loop candidates (32 loop queries x 8 candidates at the default), built from
tests/sim3_model.py's scenes (TUM1, points 1-8 m away, 1 px x scale noise, 30 % outliers,
min_inliers 20, 300 iterations, free scale), 16 distinct candidates tiled:
  loop   about 150 valid pairs among 2000 slots (what SearchByBoW leaves a loop candidate);
  dense  1000 valid pairs among 2000 slots.
Two schedules, each including the set (the constructor and SetRansacParameters):
  rounds the reference's (LoopClosing.cc:298-340): iterate(5) on the whole batch, the host
         reads found / no_more back after every round, until every candidate has returned a
         Sim3 or has no more;
  find   one call of max_iterations.
The four combinations' repeats are interleaved; each repeat times --steps schedules between two
synchronisations.  Reported: the median over repeats with min / max (ms per batch,
candidates/s, hypotheses x pairs/s over the hypotheses the kernels scored), the single host
call's latency inside the library (one iterate(5)), and parity of the first candidates with the
model.

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

WORKLOADS = {"loop": dict(n_valid=150, n_slots=2000, cap=2048), "dense": dict(n_valid=1000, n_slots=2000, cap=2048)}
ROUND = 5
OUT_I32 = ("found", "no_more", "n_inliers", "best_inliers", "best_iteration", "iterations", "n_pairs", "status")


def build(name, B, dev):
    import torch

    import sim3_model as M
    w = WORKLOADS[name]
    scenes = [M.build_scene(300 + s, **w) for s in range(16)]
    P = M.pack([scenes[b % 16] for b in range(B)])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = {k: t(P[k]) for k in ("n1", "mp1", "mp2", "oct1", "oct2", "pos", "Tcw1", "Tcw2", "draws")}
    for k in OUT_I32:
        d[k] = torch.zeros((B,), dtype=torch.int32, device=dev)
    d["inliers"] = torch.zeros((B, P["cap"]), dtype=torch.uint8, device=dev)
    d["T12"] = torch.zeros((B, 16), dtype=torch.float32, device=dev)
    d["done"] = torch.zeros((B,), dtype=torch.int32, device=dev)
    return scenes, d


def main(argv=None):
    ap = argparse.ArgumentParser(prog="sim3_bench.py")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sim3_bench.json"))
    args = ap.parse_args(argv)
    B = args.batch

    import torch

    import sim3_model as M
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver

    if not torch.cuda.is_available():
        raise SystemExit("sim3_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    cap = max(w["cap"] for w in WORKLOADS.values())
    solver = Sim3Solver(max_batch=B, cap=cap, max_iterations=300)
    # one stream of the bench's own for the library's kernels and torch's: the rounds' flag
    # arithmetic is ordered with the calls (torch's default stream would hand the library a
    # null handle, i.e. the matcher's stream)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    data = {name: build(name, B, dev) for name in WORKLOADS}

    def set_batch(name):
        sc, d = data[name]
        s0 = sc[0]
        solver.set_batch_device(d["n1"], d["mp1"], d["mp2"], d["oct1"], d["oct2"], d["pos"], d["Tcw1"], d["Tcw2"],
                                s0["level_sigma2"], s0["K1"], s0["K2"], d["draws"], fix_scale=s0["fix_scale"],
                                probability=s0["probability"], min_inliers=s0["min_inliers"],
                                max_iterations=s0["max_iterations"], stream=stream)

    def iterate(name, n):
        d = data[name][1]
        solver.iterate_batch_device(n, stream=stream, inliers=d["inliers"], T12=d["T12"], **{k: d[k] for k in OUT_I32})

    def run_find(name):
        set_batch(name)
        iterate(name, 300)
        return 1

    def run_rounds(name):
        """iterate(5) until every candidate has returned or has no more; returns the rounds."""
        d = data[name][1]
        set_batch(name)
        d["done"].zero_()
        rounds = 0
        while True:
            iterate(name, ROUND)
            rounds += 1
            d["done"] |= d["found"] | d["no_more"]
            if bool(d["done"].all().item()):   # the read-back the reference's loop makes per round
                return rounds

    combos = [(name, sched) for name in WORKLOADS for sched in ("rounds", "find")]
    runs = {"rounds": run_rounds, "find": run_find}
    nrounds = {}
    for name, sched in combos:
        for _ in range(max(1, args.warmup)):
            r = runs[sched](name)
            if sched == "rounds":
                nrounds[name] = r
    torch.cuda.synchronize(dev)
    times = {c: [] for c in combos}
    for _ in range(args.repeats):
        for c in combos:
            name, sched = c
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                runs[sched](name)
            torch.cuda.synchronize(dev)
            times[c].append((time.perf_counter() - t0) / args.steps)

    res_w = {}
    for name, (sc, d) in data.items():
        # parity of the first candidates with the model after find() (counts, flags, iterations;
        # the bench scenes are not guarded: a difference is reported, not asserted)
        run_find(name)
        torch.cuda.synchronize(dev)
        got = {k: d[k].cpu().numpy() for k in OUT_I32 + ("inliers",)}
        checked, same = min(4, B), 0
        for b in range(checked):
            s = sc[b % 16]
            r = M.run(s, ["find"])[0][0]
            same += int(all(int(got[k][b]) == int(r[k]) for k in OUT_I32)
                        and np.array_equal(got["inliers"][b, :s["n1"]], r["inliers"]))
        npairs = got["n_pairs"].astype(np.int64)
        its = np.array([M.ransac_iterations(int(n), sc[0]["min_inliers"], sc[0]["probability"],
                                            sc[0]["max_iterations"]) for n in npairs], np.int64)
        runnable = npairs >= max(3, sc[0]["min_inliers"])
        scored = {"find": int((its * npairs * runnable).sum()),
                  "rounds": int((np.minimum(its, ROUND * nrounds[name]) * npairs * runnable).sum())}
        # the single host call, inside the library: one iterate(5) after a set
        s0 = sc[0]
        n1 = s0["n1"]
        one = Sim3Solver(s0["mp1"][:n1], s0["mp2"][:n1], s0["oct1"][:n1], s0["oct2"][:n1], s0["mp_pos"], s0["Tcw1"],
                         s0["Tcw2"], s0["level_sigma2"], s0["K1"], s0["K2"], s0["fix_scale"], draws=s0["draws"],
                         matcher=None)
        us = []
        for _ in range(args.single_calls):
            one.SetRansacParameters(s0["probability"], s0["min_inliers"], s0["max_iterations"])
            one.iterate_host(ROUND)
            us.append(one.last_call_us())
        one.close()
        us = sorted(us[3:])
        entry = {"valid_pairs": int(npairs.mean()), "slots": WORKLOADS[name]["n_slots"], "cap": WORKLOADS[name]["cap"],
                 "returned": int(got["found"].sum()), "mean_iterations_to_stop": float(got["iterations"].mean()),
                 "rounds_of_5": nrounds[name],
                 "single_iterate5_us": {"median": round(statistics.median(us), 1), "min": round(us[0], 1),
                                        "max": round(us[-1], 1)},
                 "parity": {"candidates_checked": checked, "identical": same}}
        for sched in ("rounds", "find"):
            ms = sorted(1e3 * t for t in times[(name, sched)])
            med = statistics.median(ms)
            entry[sched] = {"ms_per_batch": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                            "candidates_per_s": round(B / (med * 1e-3), 1),
                            "hypotheses_x_pairs_per_s": round(scored[sched] / (med * 1e-3), 1),
                            "hypotheses_x_pairs": scored[sched]}
        res_w[name] = entry

    res = {"metric": f"candidates/s Sim3Solver, batch {B}, iterate(5) rounds, loop density",
           "value": res_w["loop"]["rounds"]["candidates_per_s"], "unit": "candidates/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True,
           "dtype": "f64", "data": "synthetic", "batch": B, "workloads": res_w,
           "kernels": {"k_sim3_setup": {"vgprs": 88}, "k_sim3_score": {"vgprs": 130, "waves_per_simd": 3},
                       "k_sim3_select": {"vgprs": 128}}}
    line = json.dumps(res)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    solver.close()


if __name__ == "__main__":
    main()
