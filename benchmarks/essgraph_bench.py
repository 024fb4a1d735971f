#!/usr/bin/env python3
"""Device OptimizeEssentialGraph on one MI355X (orbx_optimize_essential_graph_batch_device,
csrc/orbx_essgraph.hip).

    python benchmarks/essgraph_bench.py [--keyframes 1400] [--batches 1,64] [--warmup 1] [--repeats 5]
                                        [--out profiles/essgraph_bench.json]

A KITTI-00-like graph built by tests/essential_graph_model.py's scene maker: 1400 keyframes
0.3 m apart on a closed path (the sequence's 4541 frames give about that many), a spanning-tree
edge and a covisibility band of 8 per keyframe, four loop closures that reach far back, the last
10 keyframes corrected, a fixed scale (stereo), 3 points per keyframe (these figures are a
typical ORB-SLAM2 map of the sequence by reading, not measured).  The drift is make_scene's
real-loop default.  The same graph is repeated over the batch.  The batch sizes are measured
interleaved, `repeats` times each after `warmup` calls; the median is reported with min and
max.  The split between linearisation (errors, Jacobians, H and b) and the linear solves comes
from the kernel's own wall-clock ticks of problem 0, which one more call with the diagnostics
switch "essgraph_stamps" prints to stderr (100 MHz; outside the timed calls).  There is no CPU
g2o on the machine to compare with: the times are reported without a target.  One JSON line,
also written to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def stamped(call, dev):
    """One call under "essgraph_stamps": problem 0's ticks {linearisation, solve} from the line the
    library writes to stderr."""
    import torch

    from orbslam2commentedbyxcm_amd import _lib as L
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            L.debug_set("essgraph_stamps", 1)
            call()
            torch.cuda.synchronize(dev)
        finally:
            L.debug_set("essgraph_stamps", -1)
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        m = re.search(rb"essgraph_stamps: linearisation (\d+) solve (\d+)", f.read())
    return [float(m.group(1)), float(m.group(2))]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="essgraph_bench.py")
    ap.add_argument("--keyframes", type=int, default=1400)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "essgraph_bench.json"))
    args = ap.parse_args(argv)
    batches = [int(b) for b in args.batches.split(",")]

    import torch

    import essential_graph_model as M
    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer, essential_graph_envelope

    if not torch.cuda.is_available():
        raise SystemExit("essgraph_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    n = args.keyframes
    loops = ((n - 1, 0), (n - 200, n // 3), (n // 2, n // 8), (n // 4, 10))
    sc = M.make_scene(0, n, fix_scale=True, band=8, loops=loops, n_corr=10,
                      kind0=((n - 1, 0), (n - 2, 0), (n - 2, 1), (n - 3, 2)))
    blocks = essential_graph_envelope(n, sc["loop"], sc["edge_v"])
    opt = EssentialGraphOptimizer()
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    calls = {}
    for B in batches:
        P = M.pack([sc] * B)
        d = {k: t(v) for k, v in P.items()}
        out = dict(T=torch.zeros((len(P["Tcw"]), 12), dtype=torch.float32, device=dev),
                   X=torch.zeros((len(P["pos"]), 3), dtype=torch.float32, device=dev),
                   st=torch.zeros(B, dtype=torch.int32, device=dev), tr=torch.zeros((B, 2), dtype=torch.int32, device=dev),
                   chi=torch.zeros((B, 2), dtype=torch.float64, device=dev))

        def call(d=d, out=out):
            opt.essential_graph_batch_device(d["kf_off"], d["Tcw"], d["corr"], d["corr_S"], d["loop"], d["edge_off"],
                                             d["edge_v"], d["edge_kind"], d["pt_off"], d["pos"], d["pt_ref"], True, blocks,
                                             out["T"], out["X"], out["st"], d_trace=out["tr"], d_chi2=out["chi"],
                                             stream=stream)
        calls[B] = (call, out)
    for B in batches:
        for _ in range(args.warmup):
            calls[B][0]()
    torch.cuda.synchronize(dev)
    ms = {B: [] for B in batches}
    for _ in range(args.repeats):
        for B in batches:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            calls[B][0]()
            torch.cuda.synchronize(dev)
            ms[B].append((time.perf_counter() - t0) * 1e3)
    res = {"metric": "ms per call of OptimizeEssentialGraph, KITTI-00-like graph, fixed scale, 20 iterations asked",
           "vertices": n, "edges": int(len(sc["edge_v"])), "envelope_blocks": int(blocks),
           "dense_blocks": (n - 1) * n // 2, "points": int(len(sc["pos"])), "warmup": args.warmup,
           "repeats": args.repeats, "calls": {}}
    for B in batches:
        out = calls[B][1]
        ticks = np.array(stamped(calls[B][0], dev))
        tr = out["tr"].cpu().numpy()
        chi = out["chi"][0].cpu().numpy()
        assert int(out["st"].abs().sum()) == 0 and (tr == tr[0]).all()
        res["calls"][str(B)] = {"ms_median": statistics.median(ms[B]), "ms_min": min(ms[B]), "ms_max": max(ms[B]),
                                "ms_per_problem": statistics.median(ms[B]) / B, "lm_iterations": int(tr[0, 0]),
                                "linear_solves": int(tr[0, 1]), "chi2": chi.tolist(),
                                "linearisation_ms": ticks[0] / 1e5, "solve_ms": ticks[1] / 1e5,
                                "solve_share": ticks[1] / max(ticks.sum(), 1.0)}
    opt.close()
    line = json.dumps(res)
    print(line)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
