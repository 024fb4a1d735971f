"""orbx_hamming_matrix_device, orbx_window_match_device (and its host wrapper score_windows)
and orbx_compute_distinctive_descriptors_device on the GPU.

The first two are compared with plain numpy popcounts.  The window model is the reference's
sequential loop (ORBmatcher.cc:140-152): `dist < best` demotes the best to second, `else dist <
second` replaces the second.  It departs from the reference in two places, where it states the
entry point's own rule (orbx.h: "-1 if none") instead: the first candidate of a list always
takes the empty best slot, and the next one the empty second slot, so a candidate 256 away is
reported (the reference starts both distances at 256 with a strict `<` and would report
nothing; its callers threshold far below 256).  And with tie_last, where the reference keeps
no second (ORBmatcher.cc:955, `<=` on the best alone), the second slot follows the same
mirrored `<=` rule, which is what the kernel's (distance, reversed position) keys give.

Shapes: the 64 x 64 tile of the matrix kernel at 1, 63, 64, 65 and 130 rows on both sides; four
queries per workgroup at 1, 3, 4, 5 and 257 queries; candidate lists of 0, 1, 2, 63, 64, 65 and
200 entries (one lane round is 64), with a target repeated in a list, equal distances in two
neighbouring lanes and in one lane 64 positions apart, distances 0 and 256, no level table, and
the "no best" / "no second" outputs.  Every call runs on a stream of its own.

The device form of ComputeDistinctiveDescriptors must give the bytes of the host form that
test_gpu_fuse.py compares with the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 130)
LENGTHS = (0, 1, 2, 63, 64, 65, 200)
NT = 300


def popcount_matrix(a, b):
    """(na, nb) Hamming distances of 32-byte rows."""
    x = a[:, None, :] ^ b[None, :, :]
    return np.unpackbits(x, axis=2).sum(axis=2).astype(np.int32)


def descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


@pytest.fixture(scope="module")
def gpu(orbx_built):
    import torch

    from orbslam2commentedbyxcm_amd import _lib as L
    dev = torch.device("cuda", 0)
    return dict(torch=torch, L=L, lib=L.lib(), dev=dev, stream=torch.cuda.Stream(dev))


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- orbx_hamming_matrix_device ---------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix_rows():
    rng = np.random.default_rng(11)
    a, b = descriptors(rng, max(SIZES)), descriptors(rng, max(SIZES))
    a[0], b[0] = 0, 255                      # 256 apart
    b[62:66] = a[62:66]                      # identical rows across the tile edge
    a[129], b[129] = 255, 0
    return a, b


@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("na", SIZES)
def test_hamming_matrix_equals_popcounts(gpu, matrix_rows, na, nb):
    torch, s = gpu["torch"], gpu["stream"]
    a, b = matrix_rows[0][:na], matrix_rows[1][:nb]
    want = popcount_matrix(a, b)
    assert want[0, 0] == 256 and (na < 63 or nb < 63 or want[62, 62] == 0)
    with torch.cuda.stream(s):
        d_a, d_b = torch.from_numpy(a.copy()).to(gpu["dev"]), torch.from_numpy(b.copy()).to(gpu["dev"])
        d_out = torch.full((na * nb + 64,), -7, dtype=torch.int32, device=gpu["dev"])
        gpu["L"].check(gpu["lib"].orbx_hamming_matrix_device(ptr(d_a), na, ptr(d_b), nb, ptr(d_out),
                                                             C.c_void_p(s.cuda_stream)))
        got = d_out.cpu().numpy()
    assert np.array_equal(got[:na * nb].reshape(na, nb), want)
    assert (got[na * nb:] == -7).all()       # nothing past the last row


def test_hamming_matrix_empty_sides_write_nothing(gpu):
    torch, s = gpu["torch"], gpu["stream"]
    with torch.cuda.stream(s):
        d = torch.zeros((4, 32), dtype=torch.uint8, device=gpu["dev"])
        d_out = torch.full((16,), -7, dtype=torch.int32, device=gpu["dev"])
        for na, nb in ((0, 4), (4, 0), (0, 0)):
            gpu["L"].check(gpu["lib"].orbx_hamming_matrix_device(ptr(d), na, ptr(d), nb, ptr(d_out),
                                                                 C.c_void_p(s.cuda_stream)))
        assert (d_out.cpu().numpy() == -7).all()
    assert gpu["lib"].orbx_hamming_matrix_device(None, 2, ptr(d), 2, ptr(d_out), None) < 0


# ---- orbx_window_match_device -----------------------------------------------------------------
def window_model(q, t, lv, off, cand, tie_last):
    """The sequential best / second-best update over each query's list (see the module docstring
    for the two places where it is the entry point's rule, not the reference's)."""
    nq = len(off) - 1
    out = {k: np.full(nq, v, np.int32) for k, v in
           (("best_idx", -1), ("best_dist", 256), ("best_level", -1), ("second_dist", 256), ("second_level", -1))}
    for i in range(nq):
        have1 = have2 = False
        d1 = d2 = 256
        t1 = t2 = -1
        for c in cand[off[i]:off[i + 1]]:
            d = int(np.unpackbits(q[i] ^ t[c]).sum())
            if not have1 or (d <= d1 if tie_last else d < d1):
                have2, d2, t2 = have1, d1, t1
                have1, d1, t1 = True, d, int(c)
            elif not have2 or (d <= d2 if tie_last else d < d2):
                have2, d2, t2 = True, d, int(c)
        if have1:
            out["best_idx"][i], out["best_dist"][i] = t1, d1
            out["best_level"][i] = -1 if lv is None else lv[t1]
        if have2:
            out["second_dist"][i] = d2
            out["second_level"][i] = -1 if lv is None else lv[t2]
    return out


def flip(d, nbits, start=0):
    """d with bits start .. start + nbits - 1 inverted."""
    bits = np.unpackbits(d)
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


def window_problem(nq, start=0, seed=3):
    """nq queries; query i takes list length and constructed case number i + start of the cycle
    LENGTHS x 6 cases (see the module docstring).  Constructed target rows are appended to the
    random ones, each used by one query only."""
    rng = np.random.default_rng(seed)
    q = descriptors(rng, nq)
    t, lv = list(descriptors(rng, NT)), rng.integers(0, 8, NT).tolist()

    def row(d, level):
        t.append(d)
        lv.append(level)
        return len(t) - 1

    lists = []
    for i in range(nq):
        j = i + start
        n, kind = LENGTHS[j % len(LENGTHS)], (j // len(LENGTHS)) % 6
        c = rng.integers(0, NT, n).astype(np.int32)
        if n >= 2 and kind == 0:        # equal smallest distances at p and p + 1; levels differ
            p = int(rng.integers(0, n - 1))
            c[p], c[p + 1] = row(flip(q[i], 5), 2), row(flip(q[i], 5, 100), 5)
        elif n >= 65 and kind == 1:     # equal smallest distances at p and p + 64: one lane
            p = int(rng.integers(0, n - 64))
            c[p], c[p + 64] = row(flip(q[i], 7), 1), row(flip(q[i], 7, 60), 6)
        elif n >= 2 and kind == 2:      # a target repeated in the list: best and second are one row
            c[0] = c[n - 1] = row(flip(q[i], 3), 4)
        elif n >= 1 and kind == 3:      # distance 0, and 256 as the only other
            c[:] = row(~q[i], 3)
            c[n // 2] = row(q[i].copy(), 6)
        elif n >= 2 and kind == 4:      # every candidate 256 away
            c[:] = row(~q[i], 2)
        elif n >= 3 and kind == 5:      # equal second-best distances, the best between them
            c[0], c[1], c[n - 1] = row(flip(q[i], 9), 0), row(flip(q[i], 2), 3), row(flip(q[i], 9, 50), 7)
        lists.append(c)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
    cand = np.concatenate(lists).astype(np.int32)
    return q, np.stack(t), np.asarray(lv, np.int32), off, cand


# nq -> where its queries start in the cycle: 1: 200 entries with the p / p + 64 pair; 3: 64, 65
# and 200 with neighbouring ties; 4 and 257: from the empty list on
STARTS = {1: 13, 3: 4, 4: 0, 5: 9, 257: 0}


@pytest.fixture(scope="module")
def windows():
    probs = {nq: window_problem(nq, st) for nq, st in STARTS.items()}
    return {(nq, tie): (p, window_model(*p, tie)) for nq, p in probs.items() for tie in (0, 1)}


KEYS = ("best_idx", "best_dist", "best_level", "second_dist", "second_level")


def device_window_match(gpu, q, t, lv, off, cand, tie_last):
    torch, s, dev = gpu["torch"], gpu["stream"], gpu["dev"]
    nq = len(off) - 1
    with torch.cuda.stream(s):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_q, d_t, d_off = up(q), up(t), up(off)
        d_lv = None if lv is None else up(lv)
        d_c = up(cand) if len(cand) else torch.zeros(1, dtype=torch.int32, device=dev)
        d_out = torch.full((5, nq + 3), -99, dtype=torch.int32, device=dev)
        gpu["L"].check(gpu["lib"].orbx_window_match_device(
            ptr(d_q), nq, ptr(d_t), ptr(d_lv), ptr(d_off), ptr(d_c), tie_last,
            *(ptr(d_out[k]) for k in range(5)), C.c_void_p(s.cuda_stream)))
        h = d_out.cpu().numpy()
    assert (h[:, nq:] == -99).all()
    return {k: h[i, :nq] for i, k in enumerate(KEYS)}


@pytest.mark.parametrize("tie_last", [0, 1])
@pytest.mark.parametrize("nq", [1, 3, 4, 5, 257])
def test_window_match_device_equals_sequential_model(gpu, windows, nq, tie_last):
    (q, t, lv, off, cand), want = windows[(nq, tie_last)]
    got = device_window_match(gpu, q, t, lv, off, cand, tie_last)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k])[0][:8])
    nolv = device_window_match(gpu, q, t, None, off, cand, tie_last)
    for k in ("best_idx", "best_dist", "second_dist"):
        assert np.array_equal(nolv[k], want[k]), k
    assert (nolv["best_level"] == -1).all() and (nolv["second_level"] == -1).all()


@pytest.mark.parametrize("tie_last", [0, 1])
def test_score_windows_host_wrapper_equals_model(gpu, windows, tie_last):
    from orbslam2commentedbyxcm_amd.matcher import ORBmatcher
    m = ORBmatcher(0.8, False)
    for nq in (1, 5, 257):
        (q, t, lv, off, cand), want = windows[(nq, tie_last)]
        got = m.score_windows(q, t, lv, off, cand, tie_last=bool(tie_last))
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (nq, k)


def test_window_problem_holds_the_cases_it_names(windows):
    (q, t, lv, off, cand), w0 = windows[(257, 0)]
    _, w1 = windows[(257, 1)]
    n = np.diff(off)
    assert set(n.tolist()) == set(LENGTHS)
    assert (w0["best_idx"][n == 0] == -1).all() and (w0["best_dist"][n == 0] == 256).all()
    assert (w0["second_dist"][n <= 1] == 256).all() and (w0["second_level"][n <= 1] == -1).all()
    assert (w0["best_idx"][n == 1] >= 0).all()
    assert (w0["best_dist"] == 0).any() and ((w0["best_dist"] == 256) & (n >= 2)).any()
    tie = (w0["best_dist"] == w0["second_dist"]) & (n >= 2)
    assert tie.sum() >= 10
    assert (w0["best_idx"] != w1["best_idx"]).sum() >= 5          # tie_last moves the winner
    assert (w0["best_level"] != w1["best_level"]).any()
    assert (w0["second_level"] != w1["second_level"]).any()
    rep = [i for i in range(257) if n[i] >= 2 and cand[off[i]] == cand[off[i + 1] - 1]]
    assert rep
    far = [i for i in range(257) if n[i] >= 65 and w0["best_dist"][i] == w0["second_dist"][i] == 7]
    assert far                                                    # the p / p + 64 pair


# ---- orbx_compute_distinctive_descriptors_device ----------------------------------------------
def test_distinctive_descriptors_device_equals_host_form(gpu):
    from orbslam2commentedbyxcm_amd.matcher import ComputeDistinctiveDescriptors
    torch, s, dev = gpu["torch"], gpu["stream"], gpu["dev"]
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 12, 261)
    counts[:6] = [0, 1, 2, 63, 64, 130]
    counts[-1] = 0
    base = descriptors(rng, len(counts))
    rows = []
    for k, c in enumerate(counts):
        bits = np.unpackbits(np.repeat(base[k:k + 1], c, 0), axis=1)
        bits ^= (rng.random(bits.shape) < rng.uniform(0.02, 0.3)).astype(np.uint8)
        rows.append(np.packbits(bits, axis=1))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    desc = np.concatenate(rows)
    nmp = len(counts)
    best, out = ComputeDistinctiveDescriptors(off, desc)
    assert (best[counts == 0] == -1).all() and (best[counts > 0] >= 0).all()
    for with_out in (True, False):
        with torch.cuda.stream(s):
            d_off, d_desc = torch.from_numpy(off).to(dev), torch.from_numpy(desc).to(dev)
            d_best = torch.full((nmp + 5,), -9, dtype=torch.int32, device=dev)
            d_out = torch.full((nmp + 1, 32), 0xA5, dtype=torch.uint8, device=dev)
            gpu["L"].check(gpu["lib"].orbx_compute_distinctive_descriptors_device(
                nmp, ptr(d_off), ptr(d_desc), ptr(d_best), ptr(d_out) if with_out else None,
                C.c_void_p(s.cuda_stream)))
            g_best, g_out = d_best.cpu().numpy(), d_out.cpu().numpy()
        assert g_best[:nmp].tobytes() == best.tobytes() and (g_best[nmp:] == -9).all()
        has = best >= 0
        if with_out:
            assert g_out[:nmp][has].tobytes() == out[has].tobytes()
            assert g_out[:nmp][has].tobytes() == desc[off[:-1][has] + best[has]].tobytes()
            assert (g_out[:nmp][~has] == 0xA5).all() and (g_out[nmp] == 0xA5).all()
        else:
            assert (g_out == 0xA5).all()
