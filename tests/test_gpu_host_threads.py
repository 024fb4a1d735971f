"""Three host threads at once, as the reference runs Tracking, LocalMapping and LoopClosing: each
with handles of its own (created in the thread) and a torch stream of its own, released from one
barrier.  ctypes releases the GIL during a library call, so calls of different threads overlap.
Within a thread every call is followed by a synchronise of that thread's stream (uploads and
downloads are blocking): this is a check of thread safety -- handles, thread-local state and
attribute set-up from several host threads -- not of stream order, which
test_gpu_stream_order.py covers.  The roles do not make the same number of calls:

Tracking      four PoseOptimization batches
LocalMapping  a fresh CovisibilityGraph: refresh, update, LocalBA assembly, LocalBA, apply
LoopClosing   the database's score and relocalisation detection, then two essential graphs

Each thread's outputs must be the bytes of the same calls made one after the other on fresh
handles, and orbx_last_error() read in a thread must be that thread's: one ORBX_ERR_ARG is
provoked in the LoopClosing thread only.  One run; nothing is repeated.
"""
from __future__ import annotations

import threading

import numpy as np
import pytest

import stream_order as SO
import test_gpu_covisibility as CV
import test_gpu_stream_order as T

pytestmark = pytest.mark.gpu

KF_KEYS = ("score", "cand", "ncand", "loop_cand", "loop_ncand")

TRACKING = (["mono-9"], ["mixed-257"], ["mono-9", "mixed-257"], ["mixed-257"])
ESSENTIAL = ("ring-9", "ring-65")


class Work:
    """One role: make() creates its handles, calls(io) makes its calls and returns the outputs."""

    def __init__(self, role, voc=None):
        self.role, self.voc = role, voc
        self.handles = []

    def make(self):
        from orbslam2commentedbyxcm_amd import CovisibilityGraph, KeyFrameDatabase
        from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer, LocalBundleAdjuster, PoseOptimizer
        if self.role == "tracking":
            self.opt = PoseOptimizer()
            self.handles = [self.opt]
        elif self.role == "mapping":
            sc, _ = T.lm_case()
            K, cap = sc["kf_mp"].shape
            self.g, self.lba = CovisibilityGraph(K, cap, len(sc["mp_bad"]), 64), LocalBundleAdjuster()
            self.handles = [self.lba, self.g]
        else:
            self.db, self.eg = KeyFrameDatabase(self.voc, 65, 320), EssentialGraphOptimizer()
            self.handles = [self.eg, self.db]

    def calls(self, make_io):
        import test_gpu_kfdb as KF
        if self.role == "tracking":
            return [T.po_runner(self.opt, names)(make_io()) for names in TRACKING]
        if self.role == "mapping":
            return [T.lm_runner(self.g, self.lba)(make_io())]
        c = T.kf_case()
        KF.run_add(self.db, list(range(65)), c["bows"], io=make_io())
        out = [KF.run_queries(self.db, c["query"], c["ids"], c["reloc"], io=make_io(), max_cand=65)]
        return out + [T.eg_runner(self.eg, name)(make_io()) for name in ESSENTIAL]

    def close(self):
        for h in self.handles:
            h.close()


KEYS = {"tracking": [T.PO_KEYS] * 4, "mapping": [CV.CHAIN_KEYS], "closing": [KF_KEYS, T.EG_KEYS, T.EG_KEYS]}


def test_three_host_threads_give_the_serial_bytes(orbx_built):
    import torch

    import vocab_scenes as VS
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.vocabulary import ORBVocabulary
    dev = torch.device("cuda", 0)
    lib = L.lib()
    V = ORBVocabulary(0)
    assert V.loadFromText(VS.make_vocab(71, k=10, L=3).text())
    roles = ("tracking", "mapping", "closing")
    # the same calls one after the other, on handles of their own
    serial = {}
    for role in roles:
        w = Work(role, V)
        w.make()
        serial[role] = w.calls(lambda: SO.SyncIO(dev))
        w.close()
    barrier = threading.Barrier(len(roles))
    got, errors, last = {}, {}, {}

    def body(role):
        try:
            w = Work(role, V)
            w.make()
            stream = torch.cuda.Stream(dev)
            barrier.wait(timeout=60)
            with torch.cuda.stream(stream):
                got[role] = w.calls(lambda: SO.StreamIO(dev))
                if role == "closing":
                    assert lib.orbx_hamming_matrix_device(None, 2, None, 2, None, None) == L.ORBX_ERR_ARG
            last[role] = lib.orbx_last_error()
            stream.synchronize()
            w.close()
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors[role] = e
            barrier.abort()

    threads = [threading.Thread(target=body, args=(r,), name=r) for r in roles]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    V.close()
    assert not errors, errors
    for role in roles:
        assert len(got[role]) == len(serial[role]) == len(KEYS[role])
        for i, keys in enumerate(KEYS[role]):
            SO.same_bytes(got[role][i], serial[role][i], f"{role} call {i}", keys)
    assert b"bad argument" in last["closing"], last
    assert last["tracking"] == b"" and last["mapping"] == b"", last
