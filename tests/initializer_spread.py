"""Largest differences between the variants of tests/initializer_model.py over its scenes: the
SPREAD table of tests/test_gpu_initializer.py and DESIGN.md §4.19.

    python tests/initializer_spread.py
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import initializer_model as M  # noqa: E402


def main() -> None:
    worst = {}
    for name in M.ALL_SCENES:
        vs = M.scene_variants(name)
        ok, why = M.guard_for(name)
        sp = M.spreads(vs)
        a = vs[0]
        for k, v in sp.items():
            worst[k] = max(worst.get(k, 0.0), v)
        print(f"{name:14s} N {a['n_matches']:4d} model {'HF'[a['model']]} ok {a['ok']} inliers {a['n_inliers_H']:3d}/"
              f"{a['n_inliers_F']:3d} good {a['best_good']:3d}/{a['second_good']:3d} status {a['status']} "
              + " ".join(f"{k} {v:.3g}" for k, v in sp.items()) + f" guard {'ok' if ok else why}")
    print("SPREAD = {" + ", ".join(f'"{k}": {v:.3g}' for k, v in worst.items()) + "}")


if __name__ == "__main__":
    main()
