#!/usr/bin/env python3
"""How far apart correct implementations of OptimizeEssentialGraph land: the largest Tcw_opt
and pt_pos_opt entry difference, and the relative final-chi2 difference, between the variants
of tests/essential_graph_model.py (summation orders x probe roundings) over its scenes, at
each scene's exact iteration count k and at the full 20 iterations.  8 x the printed maxima are
the tolerances of tests/test_gpu_essential_graph.py (floor: 2 float32 ulps of the entry).

    python tests/essential_graph_spread.py           # guard and spread of every scene, the maxima
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_graph_model as M  # noqa: E402


def main():
    worst = {"k": [0.0, 0.0, 0.0], 20: [0.0, 0.0, 0.0]}
    for name in M.SPECS:
        k = M.exact_iterations(name)
        ok, why = M.guard(name, k)
        r = M.variants(name, k)[0]
        print(f"{name}: k {k} guard {ok} {why} trace {r['trace'].tolist()} blocks {r['blocks']} hist {r['hist'].tolist()}")
        for which, its in (("k", k), (20, 0)):
            sp = M.spread(name, its)
            print(f"    iterations {its or 20}: pose {sp[0]:.3g} position {sp[1]:.3g} chi2 (relative) {sp[2]:.3g}")
            worst[which] = [max(a, b) for a, b in zip(worst[which], sp)]
    for which in worst:
        print(f"max at {which}: pose {worst[which][0]:.3g} position {worst[which][1]:.3g} chi2 {worst[which][2]:.3g}")


if __name__ == "__main__":
    main()
