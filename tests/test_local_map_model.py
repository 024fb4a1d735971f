"""Tracking::UpdateLocalMap's model (tests/local_map_model.py) on the scenes of the GPU tests:
together they reach every branch of the reference; the ABI's argument errors and the C++ mirror's
build need no GPU."""
from __future__ import annotations

import ctypes as C
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import local_map_model as LM

ROOT = Path(__file__).resolve().parents[1]


def run_case(name, br):
    c = LM.gpu_case(name)
    g = LM.build_graph(*c["map"], c["later_bad"], c["max_conn"])
    B, mk = len(c["frame_mp"]), c["max_local_kf"]
    out = []
    for parent in c["parents"]:
        out.append(LM.update_local_map_batch(g, c["frame_mp"], c["n"], *LM.initial_lists(B, mk), mk, 10 ** 6, 10 ** 6,
                                             parent=parent, br=br))
    return g, c, out


def test_gpu_scenes_reach_every_branch():
    br = Counter()
    for name in LM.GPU_CASES:
        run_case(name, br)
    for branch in ("tie_for_maximum", "empty_counter", "bad_neighbour_skipped", "neighbour_past_tenth_ignored",
                   "child_taken", "child_after_a_bad_child", "bad_parent_appended", "parent_break",
                   "parent_break_cuts_additions", "stop_80_before_first", "stop_80_during_walk", "duplicate_votes_twice",
                   "bad_mappoint_nulled"):
        assert br[branch] >= 1, (branch, dict(br))
    assert br["capacity"] == 0


def test_empty_counter_keeps_the_old_list_and_reference():
    g, c, (w,) = run_case("band24", Counter())
    for b in (1, 2):  # all NULL; only MapPoints that nobody observes
        assert w["status"][b] == LM.EMPTY and w["ref_kf"][b] == LM.OLD_REF
        assert w["local_kf"][b, :w["local_kf_n"][b]].tolist() == list(LM.OLD_LIST)
        want = LM.update_local_points(g, list(LM.OLD_LIST))
        assert w["local_ids"][w["local_off"][b]:w["local_off"][b + 1]].tolist() == want and len(want) > 0
    assert (w["status"][3:] == 0).all() and (w["ref_kf"][3:] != LM.OLD_REF).any()


def test_the_walk_literally_on_a_hand_made_graph():
    """Five keyframes: 0 and 1 are voted (1 twice by a repeated MapPoint: pKFmax = 1, no tie); 0's
    neighbours are 1 (local) and 2; its child 3 is bad, 4 is taken; its parent is NULL.  Entry 1
    has no neighbour left, no child, and the bad parent 3: appended, and the walk ends."""
    import covisibility_model as M
    g = M.Graph(5)
    kf_mp = np.full((5, 4), -1, np.int32)
    kf_mp[0, 0] = 0
    kf_mp[1, :2] = (0, 1)
    kf_bad = np.array([0, 0, 0, 1, 0], np.uint8)
    g.refresh_observations(kf_mp, np.full(5, 4, np.int32), kf_bad, np.zeros(3, np.uint8))
    g.ordered[0], g.weights[0] = [1, 2], [20, 16]
    g.ordered[1], g.weights[1] = [0], [20]
    parent = [-1, 3, 0, 0, 0]
    br = Counter()
    fmp, local, kfmax, empty = LM.update_local_keyframes(g, np.array([1, 0, 1, -1], np.int32), 4, parent, [], br)
    assert local == [0, 1, 2, 4, 3] and kfmax == 1 and not empty
    assert br["duplicate_votes_twice"] == 1 and br["bad_parent_appended"] == 1 and br["child_after_a_bad_child"] == 1


def test_capacities_leave_the_other_frames_where_they_would_be():
    g, c, (full,) = run_case("band24", Counter())
    pick = LM.capacity_triple(full["counts"][:, 1])
    fm, n = c["frame_mp"][pick], c["n"][pick]
    nl, npts = full["counts"][pick, 0].tolist(), full["counts"][pick, 1].tolist()
    w = LM.update_local_map_batch(g, fm, n, *LM.initial_lists(3, 48), 48, 10 ** 6, npts[0] + npts[2] + 1)
    assert w["status"].tolist() == [0, LM.CAPACITY, 0] and w["local_off"].tolist() == [0, npts[0], npts[0], npts[0] + npts[2]]
    assert w["local_kf_n"].tolist() == [nl[0], 0, nl[2]] and w["ref_kf"][1] == LM.OLD_REF
    assert np.array_equal(w["frame_mp"][1], fm[1]) and not np.array_equal(full["frame_mp"][pick[1]], fm[1])
    assert w["counts"].tolist() == [[nl[0], npts[0]], [0, 0], [nl[2], npts[2]]]


def test_tally_thresholds():
    fm = np.tile(np.arange(60, dtype=np.int32), (4, 1))
    out = np.zeros((4, 60), np.uint8)
    out[1, 31:] = 1        # 31 inliers
    out[2, 29:] = 1        # 29
    out[3, 40:] = 1        # 40, recently relocalised: below 50
    obs = np.ones(60, np.int32)
    fmp, inl, ok, found = LM.tally(fm, [60] * 4, out, obs, stereo=True, recently=[0, 0, 0, 1], found=np.zeros(60, np.int32))
    assert inl.tolist() == [60, 31, 29, 40] and ok.tolist() == [1, 1, 0, 0]
    assert (fmp[1, 31:] == -1).all() and found[0] == 4 and found[59] == 1
    obs[:40] = 0
    assert LM.tally(fm, [60] * 4, out, obs)[1].tolist() == [20, 0, 0, 0]
    assert LM.tally(fm, [60] * 4, out, obs, only_tracking=True)[1].tolist() == [60, 31, 29, 40]


def test_argument_errors_need_no_gpu(orbx_built):
    """Decided before any device call, and before the graph is looked at: null pointers and
    negative sizes; a null graph."""
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced

    def upd(**kw):
        u = L.LocalMapUpdate(batch=2, cap=8, frame_mp=fake, n=fake, parent=None, max_local_kf=4, max_local_points=9,
                             max_total=9, local_kf=fake, local_kf_n=fake, ref_kf=fake, local_off=fake, local_ids=fake,
                             counts=fake, status=fake)
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def err():
        return lib.orbx_last_error().decode()

    for fn in (lambda u: lib.orbx_update_local_map_device(None, u, None), lambda u: lib.orbx_update_local_map(None, u)):
        assert fn(None) == L.ORBX_ERR_ARG
        for kw in (dict(batch=-1), dict(cap=-1), dict(max_local_kf=-1), dict(max_local_points=-2), dict(max_total=-1)):
            assert fn(C.byref(upd(**kw))) == L.ORBX_ERR_ARG and err() == "negative size", kw
        for name in ("frame_mp", "n", "local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status"):
            assert fn(C.byref(upd(**{name: None}))) == L.ORBX_ERR_ARG and err() == "null table", name
        assert fn(C.byref(upd())) == L.ORBX_ERR_ARG and err() == "null graph"
    tl = lib.orbx_track_local_map_tally_device

    def tal(**kw):
        t = L.TrackLocalMapTally(batch=2, cap=8, frame_mp=fake, n=fake, outlier=fake, n_mappoints=5, observations=fake,
                                 matches_inliers=fake, ok=fake)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    assert tl(None, None, None) == L.ORBX_ERR_ARG
    for kw in (dict(batch=-1), dict(cap=-1), dict(n_mappoints=-1)):
        assert tl(None, C.byref(tal(**kw)), None) == L.ORBX_ERR_ARG and err() == "negative size"
    for name in ("frame_mp", "n", "outlier", "observations", "matches_inliers", "ok"):
        assert tl(None, C.byref(tal(**{name: None})), None) == L.ORBX_ERR_ARG and err() == "null table", name
    assert tl(None, C.byref(tal()), None) == L.ORBX_ERR_ARG and err() == "null graph"
    so = lib.orbx_search_local_points_offsets_device
    assert so(None, None, None, None, 1, 1, None) == L.ORBX_ERR_ARG


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("localmap_cli") / "localmap_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "localmap_cli.cpp"),
                    "-o", str(out), f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"], check=True)
    return out


def test_cpp_mirror_builds_without_gpu(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


@pytest.mark.gpu
def test_cpp_update_local_map_prints_the_models_lists(exe, tmp_path):
    c = LM.gpu_case("band24")
    kf_mp, kf_n, kf_bad, mp_bad = c["map"]
    g = LM.build_graph(kf_mp, kf_n, kf_bad, mp_bad, c["later_bad"], c["max_conn"])
    K, cap = kf_mp.shape
    fm, n = c["frame_mp"][:8], c["n"][:8]
    B, mk = len(fm), c["max_local_kf"]
    lines = [f"{K} {cap} {len(mp_bad)} {c['max_conn']}"]
    lines += [f"{int(kf_n[k])} " + " ".join(str(int(p)) for p in kf_mp[k]) for k in range(K)]
    lines.append(" ".join(str(int(b)) for b in mp_bad))
    lines.append(f"{len(c['later_bad'])} " + " ".join(map(str, c["later_bad"])))
    lines.append(f"{B} {mk} 4000 20000")
    lines += [f"{int(n[b])} " + " ".join(str(int(p)) for p in fm[b]) for b in range(B)]
    path = tmp_path / "frames.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    kf0 = np.full((B, mk), -1, np.int32)
    w = LM.update_local_map_batch(g, fm, n, kf0, np.zeros(B, np.int32), np.full(B, -1, np.int32), mk, 4000, 20000)
    want = []
    for b in range(B):
        want.append(f"{b}: status {w['status'][b]} ref {w['ref_kf'][b]} kf" +
                    "".join(f" {k}" for k in w["local_kf"][b, :w["local_kf_n"][b]]))
        want.append("points" + "".join(f" {p}" for p in w["local_ids"][w["local_off"][b]:w["local_off"][b + 1]]))
        want.append("frame" + "".join(f" {p}" for p in w["frame_mp"][b]))
    assert r.stdout.splitlines() == want
    assert (w["local_kf_n"] > 5).sum() >= 5
