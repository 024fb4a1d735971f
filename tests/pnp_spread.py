"""Measures the tolerance basis of tests/test_gpu_pnp.py over its scenes:

  family A  the largest difference of any Tcw / best_Tcw entry (the float32 results) between the
            model's arithmetic variants (pnp_model.ARITH) over every call the tests make;
  family B  the largest difference of any returned Tcw entry between the convention variants
            (pnp_model.CONVENTIONS) and the model, over the convention-blind scenes.

    python tests/pnp_spread.py

prints both; 8 x each (floor: 2 float32 ulps of the entry) is the tolerance, quoted in
tests/test_gpu_pnp.py and DESIGN.md §4.21."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pnp_scenes as S  # noqa: E402


def main() -> None:
    g = {n: S.guard_for(n) for n in S.SCENES}
    a = {n: v["spread_a"] for n, v in g.items()}
    b = {n: v["spread_b"] for n, v in g.items() if "spread_b" in v}
    na, nb = max(a, key=a.get), max(b, key=b.get)
    print(f"family A: largest Tcw / best_Tcw difference over {len(a)} scenes: {a[na]:.3g} ({na})")
    print(f"family B: largest Tcw difference over {len(b)} convention-blind scenes: {b[nb]:.3g} ({nb})")
    print(f"float32 resolution at 1.0 is {np.spacing(np.float32(1.0)):.3g}")
    print("family B, refined error2 / mvMaxError: smallest distance from 1 / largest difference: "
          f"{min(v['margin_b'] for v in g.values() if 'margin_b' in v):.3g} / "
          f"{max(v['rel_b'] for v in g.values() if 'rel_b' in v):.3g}")
    print("smallest threshold margin / largest relative difference, family A: "
          f"{min(v['margin_a'] for v in g.values()):.3g} / {max(v['rel_a'] for v in g.values()):.3g}")


if __name__ == "__main__":
    main()
