#!/usr/bin/env python3
"""How far apart correct implementations of CorrectLoop's propagation and of UpdateNormalAndDepth
land: per float output, the largest entry difference between the arithmetic variants of
tests/correct_loop_model.py (float vs double Tiw * Twc, float vs double camera centre, cv::norm's
double accumulation vs float, quaternion vs matrix composition) over its scenes.  8 x a scene's
spread is that scene's tolerance in tests/test_gpu_correct_loop.py (floor: 2 float32 ulps of the
entry).

    python tests/correct_loop_spread.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import correct_loop_model as M  # noqa: E402


def main():
    worst = {k: 0.0 for k in M.FLOAT_FIELDS}
    for name in M.SCENES:
        sp = M.spread(name)
        print(f"{name}: " + " ".join(f"{k} {v:.3g}" for k, v in sp.items()))
        worst = {k: max(worst[k], sp[k]) for k in worst}
    print("max: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


if __name__ == "__main__":
    main()
