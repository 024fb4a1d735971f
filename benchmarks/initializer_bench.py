#!/usr/bin/env python3
"""Device Initializer throughput on one MI355X (orbx_initializer_*, csrc/orbx_initializer.hip;
DESIGN.md §4.19).

    python benchmarks/initializer_bench.py [--batch 256] [--steps 10] [--warmup 2] [--repeats 5]
                                           [--out profiles/initializer_bench.json]

B = --batch frame pairs built from tests/initializer_model.py's scene generator (TUM1, 0.5 px
noise, 20 % outliers): 1000 keypoints per frame, 500 of them matched, 200 iterations; 16
distinct pairs tiled, every second one planar.  Each repeat times --steps calls of
orbx_initializer_initialize_device between two synchronisations.  Reported: the median over
repeats with min / max (ms per batch, pairs/s, hypotheses x matches/s over the 2 x 200 models
scored per pair), the kernels' share of one call (torch.profiler's device times, keyed by kernel
name), the single host call's latency inside the library, and parity of the first pairs with
the model (the bench scenes are not guarded: a difference is reported, not asserted).

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

KCAP, N_MATCHED, N_KEYS, ITERATIONS = 1024, 500, 1000, 200
OUT_KEYS = ("ok", "model", "n_matches", "best_it_H", "best_it_F", "n_inliers_H", "n_inliers_F", "best_good",
            "second_good", "status")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="initializer_bench.py")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "initializer_bench.json"))
    args = ap.parse_args(argv)
    B = args.batch

    import torch

    import initializer_model as M
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    from orbslam2commentedbyxcm_amd.initializer import RESULT_LAYOUT, Initializer

    if not torch.cuda.is_available():
        raise SystemExit("initializer_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    scenes = [M.make_scene(700 + s, N=N_MATCHED, planar=bool(s & 1), extra=N_KEYS - N_MATCHED, iterations=ITERATIONS)
              for s in range(16)]
    P = dict(n1=np.zeros(B, np.int32), n2=np.zeros(B, np.int32), keys1=np.zeros((B, KCAP), KEYPOINT_DTYPE),
             keys2=np.zeros((B, KCAP), KEYPOINT_DTYPE), m12=np.full((B, KCAP), -1, np.int32),
             sets=np.zeros((B, ITERATIONS, 8), np.int32))
    for b in range(B):
        sc = scenes[b % 16]
        n1, n2 = len(sc["keys1"]), len(sc["keys2"])
        P["n1"][b], P["n2"][b] = n1, n2
        P["keys1"][b, :n1] = M.keypoints(sc["keys1"])
        P["keys2"][b, :n2] = M.keypoints(sc["keys2"])
        P["m12"][b, :n1] = sc["matches12"]
        P["sets"][b] = sc["sets"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = {k: t(P[k]) for k in ("n1", "n2", "m12", "sets")}
    d["keys1"] = t(P["keys1"].view(np.uint8).reshape(B, KCAP, 28))
    d["keys2"] = t(P["keys2"].view(np.uint8).reshape(B, KCAP, 28))
    out = {}
    for k, (dt, shape) in RESULT_LAYOUT.items():
        shp = (B,) + tuple(KCAP if x == "kcap" else x for x in shape)
        out[k] = torch.zeros(shp, dtype={"i4": torch.int32, "f4": torch.float32, "u1": torch.uint8}[dt], device=dev)
    solver = Initializer(max_batch=B, kcap=KCAP, max_iterations=ITERATIONS)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)

    def call():
        solver.initialize_batch_device(d["n1"], d["n2"], d["keys1"], d["keys2"], d["m12"], M.K4, d["sets"],
                                       stream=stream, **out)

    for _ in range(max(1, args.warmup)):
        call()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize(dev)
        times.append((time.perf_counter() - t0) / args.steps)

    # the kernels' device times over a few calls, by name
    kernels = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        calls = 3
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                call()
            torch.cuda.synchronize(dev)
        for ev in prof.key_averages():
            if "k_init" in ev.key:
                name = ev.key[ev.key.index("k_init"):].split("(")[0].split("E")[0]
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                kernels[name] = round(kernels.get(name, 0.0) + float(total) / calls, 2)
    except Exception as e:  # the profiler is optional: the per-call time above stands without it
        kernels = {"error": str(e)[:200]}

    call()
    torch.cuda.synchronize(dev)
    got = {k: out[k].cpu().numpy() for k in OUT_KEYS}
    checked, same = min(4, B), 0
    for b in range(checked):
        r = M.initialize(scenes[b % 16])
        same += int(all(int(got[k][b]) == int(r[k]) for k in OUT_KEYS))
    s0 = scenes[0]
    one = Initializer(max_batch=1, kcap=KCAP, max_iterations=ITERATIONS)
    us = []
    k1, k2 = M.keypoints(s0["keys1"]), M.keypoints(s0["keys2"])
    for _ in range(args.single_calls):
        one.initialize_host(k1, k2, s0["matches12"], M.K4, s0["sets"])
        us.append(one.last_call_us())
    one.close()
    us = sorted(us[3:])
    ms = sorted(1e3 * x for x in times)
    med = statistics.median(ms)
    scored = int(2 * ITERATIONS * got["n_matches"].astype(np.int64).sum())
    res = {"metric": f"frame pairs/s Initializer, batch {B}, {N_KEYS} keypoints, {N_MATCHED} matches, {ITERATIONS} iterations",
           "value": round(B / (med * 1e-3), 1), "unit": "pairs/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "higher_is_better": True, "dtype": "f64",
           "data": "synthetic", "batch": B,
           "ms_per_batch": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
           "us_per_pair": round(1e3 * med / B, 3),
           "hypotheses_x_matches_per_s": round(scored / (med * 1e-3), 1), "hypotheses_x_matches": scored,
           "initialized": int(got["ok"].sum()), "reconstructed_from_H": int((got["model"] == 0).sum()),
           "kernel_us_per_call": kernels,
           "single_initialize_us": {"median": round(statistics.median(us), 1), "min": round(us[0], 1),
                                    "max": round(us[-1], 1)},
           "parity": {"pairs_checked": checked, "identical": same},
           "kernels": {"k_init_normalize": {"vgprs": 34}, "k_init_hyp<16>": {"vgprs": 82, "lds_bytes": 57600},
                       "k_init_hyp<8>": {"vgprs": 112, "lds_bytes": 39168}, "k_init_score": {"vgprs": 86},
                       "k_init_select": {"vgprs": 156}, "k_init_checkrt": {"vgprs": 124},
                       "k_init_finish": {"vgprs": 124}}}
    line = json.dumps(res)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    solver.close()


if __name__ == "__main__":
    main()
