"""Measures the tolerance basis of tests/test_gpu_sim3.py: the largest difference of any
T12 / R / t / s entry between the model's variants (sim3_model.VARIANTS: eigh, Jacobi, the
eigenvector negated, reversed sums, ang and Rodrigues moved by one ulp) over every iteration
the tests walk on their scenes.

    python tests/sim3_spread.py

prints the value; 8 x it (floor: 2 float32 ulps of the entry) is the tolerance, quoted in
tests/test_gpu_sim3.py and DESIGN.md §4.16."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sim3_model as M  # noqa: E402


def spread_of(name: str) -> float:
    sc = M.scene(name)
    ok, why, st = M.guard_for(name)
    assert ok, (name, why)
    models = [M.Model(sc, v) for v in M.VARIANTS]
    worst = 0.0
    for k in range(st["upto"]):
        hs = [m.hypothesis(k)[0] for m in models]
        for key in ("T12", "R", "t", "s"):
            E = np.stack([np.asarray(h[key], np.float64).reshape(-1) for h in hs])
            fin = np.isfinite(E).all(axis=0)
            if fin.any():
                worst = max(worst, float((E[:, fin].max(axis=0) - E[:, fin].min(axis=0)).max()))
    return worst


def main() -> None:
    worst = {n: spread_of(n) for n in M.ALL_SCENES}
    name = max(worst, key=worst.get)
    print(f"largest T12 / R / t / s difference between variants over {len(worst)} scenes: {worst[name]:.3g} ({name})")
    print(f"8 x = {8 * worst[name]:.3g}; float32 resolution at 1.0 is {np.spacing(np.float32(1.0)):.3g}")


if __name__ == "__main__":
    main()
