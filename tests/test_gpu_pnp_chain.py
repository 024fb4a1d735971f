"""The middle of relocalisation (Tracking.cc:1556-1620) without a host step between the solver
and the optimiser: SearchByBoW(KF, F)'s matches feed orbx_pnp_set_batch_device, and the solver's
Tcw and frame_mp feed orbx_pose_optimization_batch_device where they lie on the device.  The
result equals the same steps through the host forms, byte for byte, and is a pose near the true one."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "benchmarks"))
import match_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu


def test_bow_matches_to_pnp_to_pose_optimization_on_the_device(oracle, orbx_built):
    import torch

    from orbslam2commentedbyxcm_amd.matcher import ORBmatcher
    from orbslam2commentedbyxcm_amd.optimizer import PoseOptimizer
    from orbslam2commentedbyxcm_amd.pnp import PnPsolver
    dx, dy = 6, 2
    A, B = S.two_views(oracle, 12, dx=dx, dy=dy)         # the candidate keyframe and the lost frame
    rng = np.random.default_rng(5)
    nA, nB = len(A.keys), len(B.keys)
    # the keyframe's MapPoints: its keypoints as the frame sees them (shifted), at random depths,
    # moved to the world by the frame's true pose
    th = 0.2
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    t = np.array([0.3, -0.1, 0.2])
    z = rng.uniform(2.0, 8.0, nA)
    Xc = np.stack([(A.keys["x"] + dx - B.cx) / B.fx * z, (A.keys["y"] + dy - B.cy) / B.fy * z, z], 1)
    pos = ((Xc - t) @ R).astype(np.float32)
    mp = np.arange(nA, dtype=np.int32)
    mp[rng.random(nA) < 0.2] = -1
    m = ORBmatcher(0.75, True)
    nm, matches = m.SearchByBoWFrame(A, mp, S.fv(A), B, S.fv(B))
    assert nm >= 15
    sig = np.asarray(B.level_sigma2, np.float32)
    K = np.array([B.fx, B.fy, B.cx, B.cy], np.float32)
    N = int(((matches >= 0) & (matches < nA)).sum())
    draws = np.stack([rng.integers(0, N - j, 300) for j in range(4)], 1).astype(np.int32)
    params = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)
    keys = np.ascontiguousarray(B.keys)

    # through the host forms
    hs = PnPsolver(keys, matches, pos, sig, K, draws=draws, matcher=m)
    hs.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    ho = hs.iterate_host(5)
    hs.close()
    assert ho["found"][0] == 1 and ho["refined"][0] == 1
    po = PoseOptimizer(matcher=m)
    inv_sig = (1.0 / sig).astype(np.float32)
    hp = po.PoseOptimization(keys, None, ho["frame_mp"], pos, inv_sig, B.fx, B.fy, B.cx, B.cy, 0.0, ho["Tcw"])

    # on the device: one stream, nothing read back in between
    dev = torch.device("cuda", m.device)
    cap = 1 << int(np.ceil(np.log2(max(nB, 2))))
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kp = np.zeros((1, cap), keys.dtype)
    kp[0, :nB] = keys
    mt = np.full((1, cap), -1, np.int32)
    mt[0, :nB] = matches
    d_kps, d_n, d_matches, d_pos = tt(kp.view(np.uint8).reshape(1, cap, 28)), tt(np.array([nB], np.int32)), tt(mt), tt(pos)
    d_draws = tt(draws[None])
    i32 = lambda: torch.zeros(1, dtype=torch.int32, device=dev)  # noqa: E731
    d_found, d_Tcw, d_mp = i32(), torch.zeros((1, 12), device=dev), torch.full((1, cap), -5, dtype=torch.int32, device=dev)
    d_opt, d_out, d_ninl, d_ninit = torch.zeros((1, 12), device=dev), torch.zeros((1, cap), dtype=torch.uint8, device=dev), \
        i32(), i32()
    ds = PnPsolver(matcher=m, max_batch=1, cap=cap, max_draws=300)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ds.set_batch_device(d_kps, d_n, d_matches, d_pos, sig, K, d_draws, stream=stream, **params)
        ds.iterate_batch_device(5, stream=stream, found=d_found, Tcw=d_Tcw, frame_mp=d_mp)
        po.pose_optimization_batch_device(d_kps, d_n, d_mp, d_pos, inv_sig, B.fx, B.fy, B.cx, B.cy, 0.0, d_Tcw, d_opt,
                                          d_out, d_ninl, d_ninit, stream=stream)
    stream.synchronize()
    assert int(d_found[0]) == 1
    assert d_Tcw.cpu().numpy().tobytes() == ho["Tcw"].tobytes()
    assert np.array_equal(d_mp.cpu().numpy()[0, :nB], ho["frame_mp"])
    assert d_opt.cpu().numpy().tobytes() == hp["Tcw"].tobytes()
    assert np.array_equal(d_out.cpu().numpy()[0, :nB], hp["outlier"]) and int(d_ninl[0]) == hp["ninliers"]
    # not a garbage pose.  An inlier's keypoint lies within sqrt(th2 sigma2) px of its projection, at most
    # sqrt(5.991 * 1.2^14) = 8.8 px at the top level, a bearing error of 8.8 / 500 = 0.018 rad; a pose fitted to
    # ten or more such bearings stays within a few times that of the truth: 5 x for the rotation entries, and
    # 5 x that bearing at the largest depth (8 m) for the translation.  A wrong pose is off by O(1).
    bearing = np.sqrt(5.991 * float(sig.max())) / min(B.fx, B.fy)
    T = hp["Tcw"].reshape(3, 4)
    assert np.abs(T[:, :3] - R).max() < 5 * bearing and np.abs(T[:, 3] - t).max() < 5 * bearing * 8.0
    assert hp["ninliers"] >= 10
    ds.close()
    po.close()
    m.close()
