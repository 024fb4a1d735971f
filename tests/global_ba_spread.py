#!/usr/bin/env python3
"""How far apart correct implementations of Optimizer::BundleAdjustment land: per scene of
tests/test_gpu_global_ba.py the largest pose-entry and position-entry difference between the
variants of tests/global_ba_model.py (summation orders, the 3x3 inverse, the order of the
factorisation).  8 x a scene's figures are that scene's tolerances in the GPU test (floor: 2
float32 ulps of the entry).

    python tests/global_ba_spread.py           # guard and spread of every scene, the maxima
    python tests/global_ba_spread.py --find    # for every scene the first seed that passes its guard
"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import global_ba_model as G  # noqa: E402


def main():
    find = "--find" in sys.argv
    worst_T = worst_X = 0.0
    for name in G.SPECS:
        seeds = range(64) if find else [G.SEEDS[name]]
        t0 = time.time()
        for seed in seeds:
            try:
                sc = G.scene(name, seed)
            except AssertionError:
                continue
            vs = G.variants(sc, G.SPECS[name][4], **G.params(name))
            ok, why = G.guard(vs)
            if ok or not find:
                break
        dT, dX = G.spread(vs)
        K, F = len(sc["fixed"]), len(vs[0]["active_kf"][0]) if vs[0]["active_kf"] else 0
        print(f"{name:12s} seed {seed:3d} guard {'ok ' if ok else 'NO '} pose {dT:.3g} position {dX:.3g} "
              f"trace {vs[0]['trace'].tolist()} stop {vs[0]['stop']} kf {K} columns {F} blocks {vs[0]['blocks']} "
              f"of {F * (F + 1) // 2} chi2 {vs[0]['chi2'][0]:.6g} -> {vs[0]['chi2'][1]:.6g}  {why}  "
              f"[{time.time() - t0:.1f} s]", flush=True)
        if ok:
            worst_T, worst_X = max(worst_T, dT), max(worst_X, dX)
    print(f"largest pose-entry spread {worst_T:.3g}, largest position-entry spread {worst_X:.3g}")


if __name__ == "__main__":
    main()
