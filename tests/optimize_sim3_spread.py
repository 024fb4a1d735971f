#!/usr/bin/env python3
"""How far apart correct implementations of OptimizeSim3 land: the largest R12 / t12 / s12
entry difference between the model's variants (four summation orders x three probe exp()
roundings) over the scenes of tests/test_gpu_optimize_sim3.py.  8 x the printed figure is that
test's tolerance (S12_SPREAD there).

    python tests/optimize_sim3_spread.py           # guard and spread of every scene, the maximum
    python tests/optimize_sim3_spread.py --find    # for every scene the first seed that passes
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import optimize_sim3_model as M  # noqa: E402


def check(name, seed=None):
    sc = M.scene(name, seed)
    vs = M.variants(sc)
    ok, why = M.guard(vs)
    extra = ok and bool(M.scene_extra(name, vs[0]))
    return ok and extra, why if ok else why, vs


def main(argv):
    if "--find" in argv:
        for name in M.ALL_SCENES:
            for seed in range(200):
                ok, why, vs = check(name, seed)
                if ok:
                    print(f'    "{name}": {seed},   # {why}; decisions {M.decision_margin(vs):.3g}; '
                          f"trace {vs[0]['trace'].reshape(-1).tolist()}", flush=True)
                    break
            else:
                print(f"    # {name}: no seed below 200 passes ({why})", flush=True)
        return 0
    worst, bad = 0.0, 0
    for name in M.ALL_SCENES:
        ok, why, vs = check(name)
        sp = M.s12_spread(vs)
        r = vs[0]
        print(f"{name:18s} {'ok ' if ok else 'BAD'} ncorr {r['ncorr']:4d} nbad {r['nbad']:3d} nin {r['ninliers']:4d} "
              f"trace {r['trace'].reshape(-1).tolist()} spread {sp:.3g}  {why}", flush=True)
        bad += not ok
        if ok:
            worst = max(worst, sp)
    print(f"largest S12 entry spread over the passing scenes: {worst:.3g}; scenes failing: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
