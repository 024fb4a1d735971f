#!/usr/bin/env python3
"""Device CreateNewMapPoints triangulation on one MI355X (orbx_triangulate_pairs_batch_device,
csrc/orbx_triangulate.hip).

    python benchmarks/triangulate_bench.py [--batch 64] [--nn 10] [--steps 10] [--warmup 3]
                                           [--repeats 5] [--out profiles/triangulate_bench.json]

Two measurements on the keyframe bench's own plan (bench.py --workload euroc: 64 stereo
keyframes, nn 10, 414 keyframe pairs after the baseline skip):

* the call alone: on the matched pairs one pipeline step left in HBM, --steps calls between two
  synchronisations, --repeats times; median with min / max, us per call (= per step);
* the keyframe pipeline's step with and without triangulate=True: two pipelines on the same
  input, their repeats interleaved (off, on, off, on, ...), --steps steps each between two
  synchronisations; medians, the change in percent of the triangulate=False leg, and that
  leg's own run-to-run spread (max - min over its repeats) to judge the change against.

Prints ONE JSON line and writes it to --out.  Nobody has measured this kernel before, so no
target is set: the file is the record.
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


def main(argv=None):
    ap = argparse.ArgumentParser(prog="triangulate_bench.py")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nn", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulate_bench.json"))
    args = ap.parse_args(argv)
    if args.repeats < 5:
        raise SystemExit("at least five interleaved pairs")

    import torch

    from orbslam2commentedbyxcm_amd import ORBextractor, synth
    from orbslam2commentedbyxcm_amd.keyframes import EUROC as s
    from orbslam2commentedbyxcm_amd.keyframes import StereoKeyFramePipeline

    if not torch.cuda.is_available():
        raise SystemExit("triangulate_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    # the keyframe bench's vocabulary: level-1 centres from the stream's first left view
    seq0 = synth.StereoSequence(3, 1, s["width"], s["height"], step=16, margin=256, disp=13)
    ex0 = ORBextractor(s["nfeatures"], s["scale"], s["nlevels"], s["ini_th"], s["min_th"], device=0)
    _, d0 = ex0(seq0.views([0])[0][0])
    ex0.close()
    text = synth.vocabulary_text(7, 10, 6, 0, 0, centres=d0)
    pls = {flag: StereoKeyFramePipeline(args.batch, nn=args.nn, vocab_text=text, triangulate=flag)
           for flag in (False, True)}
    for pl in pls.values():
        pl.run(max(args.warmup, 2))
    torch.cuda.synchronize(dev)

    step_s = {flag: [] for flag in pls}
    for _ in range(args.repeats):
        for flag, pl in pls.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            pl.run(args.steps)
            torch.cuda.synchronize(dev)
            step_s[flag].append((time.perf_counter() - t0) / args.steps)

    # the call alone, on the newest step's pairs
    pl = pls[True]
    k = pl.last
    res = pl.host_results()
    P = len(pl.plan.pairs)
    stream = pl.ts

    def call():
        pl.tg.triangulate_pairs_batch_device(pl._gtabs[k], pl.cam, pl._geom_pairs, pl.cap, pl.tri_pairs[k], pl.tri_n[k],
                                             pl.new_points[k], stream=stream)

    for _ in range(max(args.warmup, 2)):
        call()
    torch.cuda.synchronize(dev)
    call_s = []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize(dev)
        call_s.append((time.perf_counter() - t0) / args.steps)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_us = []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        ev0.record(stream)
        call()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        dev_us.append(1e3 * ev0.elapsed_time(ev1))

    matched = int(res["tri_n"].sum())
    reasons = np.bincount(np.concatenate([res["new_reason"][p, :res["tri_n"][p]] for p in range(P)]), minlength=10)
    methods = np.bincount(np.concatenate([res["new_method"][p, :res["tri_n"][p]] for p in range(P)]), minlength=4)
    for p_ in pls.values():
        p_.close()

    def summary(xs, scale):
        xs = sorted(scale * x for x in xs)
        return {"median": round(statistics.median(xs), 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}

    off, on = summary(step_s[False], 1e3), summary(step_s[True], 1e3)
    change = 100.0 * (on["median"] - off["median"]) / off["median"]
    spread = 100.0 * (off["max"] - off["min"]) / off["median"]
    call_us = summary(call_s, 1e6)
    out = {"metric": f"us per orbx_triangulate_pairs_batch_device call, {P} keyframe pairs, {matched} matched pairs",
           "value": call_us["median"], "unit": "us", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "higher_is_better": False, "dtype": "f64", "data": "synthetic",
           "batch": args.batch, "nn": args.nn, "keyframe_pairs": P, "matched_pairs": matched,
           "new_points": int(res["new_nnew"].sum()), "reasons": reasons.tolist(), "methods": methods.tolist(),
           "call_us_per_step": call_us, "call_device_us_single": summary(dev_us, 1.0),
           "matched_pairs_per_s": round(matched / (call_us["median"] * 1e-6), 1),
           "pipeline_step_ms": {"triangulate_false": off, "triangulate_true": on,
                                "change_percent_of_false_leg": round(change, 2),
                                "false_leg_spread_percent": round(spread, 2)},
           "keyframes_per_s": {"triangulate_false": round(args.batch / (off["median"] * 1e-3), 1),
                               "triangulate_true": round(args.batch / (on["median"] * 1e-3), 1)},
           "kernels": {"k_triangulate_pairs": {"threads": 256, "vgprs": 174, "agprs": 0, "sgprs": 106,
                                               "scratch_bytes": 0, "lds_bytes": 16, "waves_per_simd": 2}}}
    line = json.dumps(out)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
