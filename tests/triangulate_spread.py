"""Largest pos / normal / distance difference between the variants of tests/triangulate_model.py
over its scenes: the X3D_SPREAD of tests/test_gpu_triangulate.py.

    python tests/triangulate_spread.py
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import triangulate_model as M  # noqa: E402


def main() -> None:
    worst = 0.0
    for name in M.ALL_SCENES:
        vs = M.scene_variants(name)
        ok, why = M.guard(vs)
        s = M.x3d_spread(vs)
        worst = max(worst, s)
        n = sum(len(r["reason"]) for r in vs[0])
        print(f"{name:12s} pairs {n:5d} accepted {sum(r['nnew'] for r in vs[0]):5d} spread {s:.3g} guard {'ok' if ok else why}")
    reasons, methods = M.histogram()
    print("reasons", reasons.tolist(), "methods", methods.tolist(), "scene_extra", M.scene_extra())
    print(f"X3D_SPREAD = {worst:.3g}")


if __name__ == "__main__":
    main()
