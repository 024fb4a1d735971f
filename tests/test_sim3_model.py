"""tests/sim3_model.py, the parity basis of orbx_sim3_*, checked on the CPU: against a second,
deliberately sequential transcription of Sim3Solver::iterate (src/Sim3Solver.cc:188-274, with
ComputeSim3 / CheckInliers / Project written out point by point), the closed-form draw mapping
against the literal list, the truncated thresholds and the iteration table's known answers,
and the guard of every scene the GPU tests use."""
from __future__ import annotations

import itertools
import math

import numpy as np
import pytest

import sim3_model as M


class Sequential:
    """Sim3Solver as the reference writes it: one object, member state, a loop per point; the
    eigenvector from numpy.linalg.eigh like cv::eigen's, largest eigenvalue first."""

    def __init__(self, sc):
        self.sc = sc
        self.mN1 = int(sc["n1"])
        n_mp = len(sc["mp_pos"])
        T1 = np.asarray(sc["Tcw1"], np.float32).astype(np.float64).reshape(3, 4)
        T2 = np.asarray(sc["Tcw2"], np.float32).astype(np.float64).reshape(3, 4)
        self.mvX3Dc1, self.mvX3Dc2, self.mvnIndices1, self.mvnMaxError1, self.mvnMaxError2 = [], [], [], [], []
        nl = len(sc["level_sigma2"])
        for i1 in range(self.mN1):                                   # cc:67-116
            a, b = int(sc["mp1"][i1]), int(sc["mp2"][i1])
            if not (0 <= a < n_mp and 0 <= b < n_mp):
                continue
            s1 = np.float32(sc["level_sigma2"][min(max(int(sc["oct1"][i1]), 0), nl - 1)])
            s2 = np.float32(sc["level_sigma2"][min(max(int(sc["oct2"][i1]), 0), nl - 1)])
            self.mvnMaxError1.append(int(9.210 * float(s1)))
            self.mvnMaxError2.append(int(9.210 * float(s2)))
            self.mvnIndices1.append(i1)
            X1 = np.asarray(sc["mp_pos"][a], np.float32).astype(np.float64)
            X2 = np.asarray(sc["mp_pos"][b], np.float32).astype(np.float64)
            self.mvX3Dc1.append(self._rt(T1, X1))
            self.mvX3Dc2.append(self._rt(T2, X2))
        self.N = len(self.mvnIndices1)
        self.mvP1im1 = [self._img(X, sc["K1"]) for X in self.mvX3Dc1]
        self.mvP2im2 = [self._img(X, sc["K2"]) for X in self.mvX3Dc2]
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best_iteration = -1
        self.mRansacMinInliers = sc["min_inliers"]
        self.mRansacMaxIts = M.ransac_iterations(self.N, sc["min_inliers"], sc["probability"], sc["max_iterations"])

    @staticmethod
    def _rt(T, X):
        return [((T[r][0] * X[0] + T[r][1] * X[1]) + T[r][2] * X[2]) + T[r][3] for r in range(3)]

    @staticmethod
    def _img(X, K):
        K = [float(np.float32(k)) for k in K]
        with np.errstate(all="ignore"):
            invz = float(np.float64(1.0) / np.float64(X[2]))
        return [K[0] * (X[0] * invz) + K[2], K[1] * (X[1] * invz) + K[3]]

    def iterate(self, nIterations):
        vbInliers = [False] * self.mN1
        if self.N < self.mRansacMinInliers or self.N < 3:
            return None, True, vbInliers, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            cur += 1
            k = self.mnIterations
            self.mnIterations += 1
            avail = list(range(self.N))
            P1, P2 = [], []
            for j in range(3):
                randi = int(self.sc["draws"][k][j])
                idx = avail[randi]
                P1.append(self.mvX3Dc1[idx])
                P2.append(self.mvX3Dc2[idx])
                avail[randi] = avail[-1]
                avail.pop()
            h = M.horn(P1, P2, self.sc["fix_scale"], "eigh")
            flags, n = [], 0
            for i in range(self.N):
                with np.errstate(all="ignore"):
                    q = self._img(self._rt(h["T12"], self.mvX3Dc2[i]), self.sc["K1"])
                    p = self._img(self._rt(h["T21"], self.mvX3Dc1[i]), self.sc["K2"])
                d1 = [self.mvP1im1[i][0] - q[0], self.mvP1im1[i][1] - q[1]]
                d2 = [p[0] - self.mvP2im2[i][0], p[1] - self.mvP2im2[i][1]]
                e1, e2 = d1[0] * d1[0] + d1[1] * d1[1], d2[0] * d2[0] + d2[1] * d2[1]
                ok = e1 < self.mvnMaxError1[i] and e2 < self.mvnMaxError2[i]
                flags.append(ok)
                n += int(ok)
            if n >= self.mnBestInliers:
                self.mnBestInliers, self.best_iteration, self.mBestT12 = n, k, h["T12"]
                if n > self.mRansacMinInliers:
                    for i in range(self.N):
                        if flags[i]:
                            vbInliers[self.mvnIndices1[i]] = True
                    return h["T12"], False, vbInliers, n
        return None, self.mnIterations >= self.mRansacMaxIts, vbInliers, 0


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_sequential_transcription(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(4, 90))
    sc = M.build_scene(7000 + seed, n_valid=n, cap=128, fix_scale=bool(seed % 2), outliers=float(rng.uniform(0, 0.7)),
                       min_inliers=int(rng.integers(3, 25)), max_iterations=40)
    a, b = M.Model(sc, "eigh"), Sequential(sc)
    assert b.N == a.S["N"] and b.mRansacMaxIts == a.S["max_its"]
    for step in itertools.islice(itertools.cycle((1, 5, 3, 40)), 30):
        r = a.iterate(step)
        T, no_more, flags, nin = b.iterate(step)
        assert (T is not None) == bool(r["found"]) and no_more == bool(r["no_more"]) and nin == r["n_inliers"]
        assert np.array_equal(np.array(flags, np.uint8), r["inliers"])
        assert (a.iterations, a.best_inliers, a.best_iteration) == (b.mnIterations, b.mnBestInliers, b.best_iteration)
        if T is not None:
            assert np.array_equal(T, r["T12"])
        if no_more and not r["found"]:
            break


@pytest.mark.parametrize("n", [3, 4, 5])
def test_closed_form_draws_equal_the_literal_list(n):
    count = 0
    for r in itertools.product(range(n), range(max(1, n - 1)), range(max(1, n - 2))):
        assert M.draws_valid(n, r)
        got, want = M.draw_indices_closed(n, r), M.draw_indices_list(n, r)
        assert got == want, (n, r, got, want)
        assert len(set(got)) == 3
        count += 1
    assert count == n * (n - 1) * (n - 2)


def test_draws_outside_their_range_are_invalid():
    assert not M.draws_valid(5, (5, 0, 0)) and not M.draws_valid(5, (0, 4, 0)) and not M.draws_valid(5, (0, 0, 3))
    assert not M.draws_valid(5, (-1, 0, 0)) and M.draws_valid(5, (4, 3, 2))


def test_thresholds_are_truncated_integers():
    """mvnMaxError is a vector<size_t> (Sim3Solver.h:143-144): 9.210 * 1.2^(2 level), truncated."""
    thr = M.thresholds(M.LEVEL_SIGMA2)
    assert thr.tolist() == [9.0, 13.0, 19.0, 27.0, 39.0, 57.0, 82.0, 118.0]
    assert thr.tolist() == [float(math.floor(9.210 * 1.2 ** (2 * l))) for l in range(8)]


def test_iteration_table_known_answers():
    assert M.ransac_iterations(100, 20, 0.99, 300) == 300
    assert M.ransac_iterations(25, 20, 0.99, 300) == 7
    assert M.ransac_iterations(20, 20, 0.99, 300) == 1
    assert M.ransac_iterations(19, 20, 0.99, 300) == 1      # never used: no more at once
    assert M.ransac_iterations(100, 20, 0.99, 50) == 50
    assert all(M.ransac_iterations(n, 20, 0.99, 300) >= 1 for n in range(0, 1025))


def test_jacobi_finds_the_largest_eigenvector():
    rng = np.random.default_rng(3)
    for _ in range(50):
        A = rng.normal(size=(4, 4))
        A = A + A.T
        q = np.array(M.jacobi4(A))
        w, V = np.linalg.eigh(A)
        assert abs(abs(q @ V[:, 3]) - 1.0) < 1e-12
    assert M.jacobi4(np.diag([3.0, 1.0, 2.0, -1.0])) == [1.0, 0.0, 0.0, 0.0]   # exact zeros: no rotation


def test_identical_point_sets_give_nan():
    """cc:371: |v| == 0 exactly, 0/0, NaN ever after; 0 inliers, and the best state is NaN."""
    sc = M.scene("nan-50")
    for v in M.VARIANTS:
        m = M.Model(sc, v)
        r = m.find()
        assert r["no_more"] == 1 and r["found"] == 0 and r["best_inliers"] == 0
        assert r["best_iteration"] == r["iterations"] - 1 == sc["max_iterations"] - 1
        assert np.isnan(r["best_R"]).all() and np.isnan(r["best_t"]).all() and math.isnan(r["best_s"])


def test_schedules_agree_in_the_model():
    for name in M.CHUNK_SCENES:
        sc = M.scene(name)
        five, one = M.rounds_of(sc, 5)[-1], M.rounds_of(sc, 1)[-1]
        whole = M.run(sc, ["find"])[0][0]
        for k in ("found", "no_more", "n_inliers", "best_inliers", "best_iteration", "iterations"):
            assert five[k] == one[k] == whole[k], (name, k)
        assert np.array_equal(five["inliers"], whole["inliers"]) and np.array_equal(one["inliers"], whole["inliers"])


def test_scene_roles():
    """The scenes the GPU tests name for a behaviour have it."""
    first = M.run(M.scene("first-64"), ["find"])[0][0]
    assert first["found"] == 1 and first["iterations"] == 1
    late = M.run(M.scene("late-100"), ["find"])[0][0]
    assert late["found"] == 1 and late["iterations"] > 20
    for name in ("exhaust-40", "exhaust-25"):
        r = M.run(M.scene(name), ["find"])[0][0]
        assert r["found"] == 0 and r["no_more"] == 1, name
    assert M.run(M.scene("exhaust-25"), ["find"])[0][0]["iterations"] == 7
    rs, _ = M.run(M.scene("continue-300"), M.SCHEDULES["continue-300"])
    assert rs[0]["found"] == 1 and rs[0]["iterations"] < 300
    for a, b in zip(rs, rs[1:]):                    # a later return needs inl >= the best so far
        if b["found"]:
            assert b["n_inliers"] >= a["best_inliers"]
    assert any(b["found"] for b in rs[1:])


@pytest.mark.parametrize("name", M.ALL_SCENES)
def test_every_gpu_scene_holds_its_guard(name):
    ok, why, _ = M.guard_for(name)
    assert ok, (name, why)
