#!/usr/bin/env python3
"""How far apart correct implementations of LocalBundleAdjustment land: the largest pose-entry
and position-entry difference between the variants of tests/local_ba_model.py (summation
orders, the 3x3 inverse, the order of the factorisation) over the scenes of
tests/test_gpu_local_ba.py.  8 x the printed figures are that test's tolerances (floor: 2
float32 ulps of the entry).

    python tests/local_ba_spread.py           # guard and spread of every scene, the maxima
    python tests/local_ba_spread.py --find    # for every scene the first seed that passes its guard
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import local_ba_model as M  # noqa: E402


def main():
    find = "--find" in sys.argv
    worst_T = worst_X = 0.0
    for name in M.SPECS:
        seeds = range(64) if find else [M.SEEDS[name]]
        for seed in seeds:
            try:
                vs = M.variants(M.scene(name, seed))
            except AssertionError:
                continue
            ok, why = M.guard(vs)
            ok = ok and M.scene_extra(name, vs[0])
            if ok or not find:
                break
        dT, dX = M.spread(vs)
        print(f"{name:18s} seed {seed:3d} guard {'ok ' if ok else 'NO '} pose {dT:.3g} position {dX:.3g} "
              f"trace {vs[0]['trace'].reshape(-1).tolist()} n_erase {vs[0]['n_erase']}  {why}")
        if ok:
            worst_T, worst_X = max(worst_T, dT), max(worst_X, dX)
    print(f"largest pose-entry spread {worst_T:.3g}, largest position-entry spread {worst_X:.3g}")


if __name__ == "__main__":
    main()
