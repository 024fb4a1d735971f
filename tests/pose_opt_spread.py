"""Measures, on the CPU, the scale of legitimate differences in PoseOptimization's pose over
the scenes of tests/test_gpu_pose_opt.py: the largest pose-entry difference (before the
rounding to float) between the three summation orders of tests/pose_opt_model.py.  The GPU
test's tolerance is 8 x this spread (floor: 2 float32 ulps of the entry).

    python tests/pose_opt_spread.py          # the spread and each scene's guard
    python tests/pose_opt_spread.py --find   # the first seed per scene for which guard() holds
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_opt_model as M  # noqa: E402


def find(limit=120):
    """Per scene the first seed whose guard() holds and whose LM decisions are 1000 x (else
    10 x, else at all) above their spread between the variants."""
    seeds = {}
    for name in M.scene_specs():
        best = {}
        for seed in range(limit):
            vs = M.variants(M.scene(name, seed))
            if not M.guard(vs)[0] or not M.scene_extra(name, vs[0]):
                continue
            dm = M.decision_margin(vs)
            tier = 0 if dm > 1000.0 else (1 if dm > 10.0 else 2)
            best.setdefault(tier, seed)
            if tier == 0:
                break
        if not best:
            raise SystemExit(f"no seed below {limit} for {name}")
        tier = min(best)
        seeds[name] = best[tier]
        print(f'    "{name}": {seeds[name]},  # tier {tier}', flush=True)
    return seeds


def measure():
    worst = 0.0
    for name in M.scene_specs():
        vs = M.variants(M.scene(name))
        ok, why = M.guard(vs)
        sp = M.pose_spread(vs)
        worst = max(worst, sp)
        print(f"{name:16s} guard={ok} ({why}) pose spread {sp:.3g} trace {vs[0]['trace'].tolist()}")
    print(f"largest pose-entry spread: {worst:.3g}; 8 x = {8 * worst:.3g}")
    return worst


if __name__ == "__main__":
    if "--find" in sys.argv:
        find()
    else:
        measure()
