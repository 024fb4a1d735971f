"""The rig of the stream-order tests (test_gpu_stream_order.py, test_gpu_host_threads.py).

The device entry points are documented as asynchronous on the caller's stream.  A test that
uploads with a blocking copy, synchronises the device around the call and uses the null stream
cannot see a launch on the wrong stream, a host table read after the call returned, a work area
reused too early or a stream switch that does not wait.  This module lets a runner of the
existing GPU tests be driven in two ways through one I/O object:

SyncIO     what the tests always did: blocking uploads, a device synchronise before and after
           the call, the current stream.  It also times the calls: with an event pair on that
           stream and, because the null stream's handle is 0 and the library then runs on the
           handle's own stream, which those events do not bracket, by the host's clock from the
           synchronise before to the one after.  call_ms is the larger.
OrderedIO  a *held* stream: device inputs are first filled with a decoy (a blocking upload),
           then a hold (torch.cuda._sleep, or a chain of matmuls where that is unusable) goes
           onto a fresh stream, and behind it, in this order, the real inputs from pinned host
           memory, the library call(s) with that stream, and the outputs into pinned host
           memory.  Only that stream is synchronised.  Anything the library does out of stream
           order runs while the hold is still running and sees the decoy.

Decoys keep a misordered run wrong rather than faulting: a decoy has the real input's shapes,
its index and offset arrays are the real ones, and only payloads differ (check_decoy;
tests/test_stream_order_decoys.py applies it to every decoy the GPU tests use).

Several HIP streams can share one hardware queue, and then run in submission order: a
wrong-stream launch would be ordered by accident.  probe() therefore proves, before a module's
tests, that a violation is visible: behind a hold with the real uploads queued, one call on
the handle's own stream (stream=None) must give the bytes of a synchronous run on the decoy.
"""
from __future__ import annotations

import contextlib
import time

import numpy as np

HOLD_FACTOR = 20          # hold >= 20 x the GPU time of the synchronous run of the same calls
HOLD_MIN_MS = 50.0
HOLD_MAX_MS = 1000.0
PROBE_STREAMS = 8

_rate = {}                # device index -> ("sleep", cycles per ms) | ("matmul", matmuls per ms, matrix)


def _calibrate(dev):
    """Once per process and device: how many _sleep cycles (or matmuls) make a millisecond."""
    import torch
    if dev.index in _rate:
        return _rate[dev.index]
    s = torch.cuda.Stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 20_000_000
    kind = None
    if hasattr(torch.cuda, "_sleep"):
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)            # loads the kernel
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        s.synchronize()
        ms = e0.elapsed_time(e1)
        if ms > 1.0:                           # a spin too short to time is not a usable hold
            kind = ("sleep", cycles / ms, None)
    if kind is None:
        with torch.cuda.stream(s):
            a = torch.ones((2048, 2048), dtype=torch.float32, device=dev)
            torch.mm(a, a)
            e0.record()
            for _ in range(20):
                torch.mm(a, a)
            e1.record()
        s.synchronize()
        kind = ("matmul", 20 / max(e0.elapsed_time(e1), 1e-3), a)
    _rate[dev.index] = kind
    print(f"stream_order: hold by {kind[0]}, {kind[1]:.4g} per ms")
    return kind


def hold_ms_for(call_ms, floor_ms=HOLD_MIN_MS):
    return float(min(HOLD_MAX_MS, max(floor_ms, HOLD_MIN_MS, HOLD_FACTOR * call_ms)))


def enqueue_hold(stream, dev, ms):
    """Keep `stream` busy for about `ms` milliseconds of GPU time."""
    import torch
    kind, per_ms, a = _calibrate(dev)
    with torch.cuda.stream(stream):
        if kind == "sleep":
            torch.cuda._sleep(int(per_ms * ms))
        else:
            for _ in range(max(1, int(per_ms * ms))):
                torch.mm(a, a)


class SyncIO:
    """Today's behaviour of the GPU tests; the default of every runner."""
    ordered = False

    def __init__(self, dev):
        import torch
        self.torch, self.dev = torch, dev
        self.call_ms = 0.0
        self._e0 = None

    def up(self, real, decoy=None):
        return self.torch.from_numpy(np.ascontiguousarray(real)).to(self.dev)

    def put(self, dst, real, decoy=None):
        """Fill an existing device tensor (an in/out table that lives in a handle's wrapper)."""
        dst.copy_(self.torch.from_numpy(np.ascontiguousarray(real).reshape(tuple(dst.shape))).to(self.dev))
        return dst

    def full(self, shape, value, dtype):
        return self.torch.full(shape, value, dtype=dtype, device=self.dev)

    def host(self, real, decoy=None):
        return real

    def on_stream(self):
        """The context in which a wrapper that allocates its own outputs is called."""
        return contextlib.nullcontext()

    @property
    def stream(self):
        return self.torch.cuda.current_stream(self.dev)

    @property
    def stream_ptr(self):
        return self.stream.cuda_stream

    def begin(self):
        torch = self.torch
        torch.cuda.synchronize(self.dev)
        self._e0 = torch.cuda.Event(enable_timing=True)
        self._e0.record(self.stream)
        self._t0 = time.perf_counter()

    def end(self):
        e1 = self.torch.cuda.Event(enable_timing=True)
        e1.record(self.stream)
        self.torch.cuda.synchronize(self.dev)
        self.call_ms += max(self._e0.elapsed_time(e1), 1e3 * (time.perf_counter() - self._t0))

    def down(self, t):
        return None if t is None else t.cpu().numpy()

    def finish(self):
        pass


class StreamIO(SyncIO):
    """Blocking uploads and downloads on the current stream; no device-wide synchronise."""

    def begin(self):
        self._e0 = self.torch.cuda.Event(enable_timing=True)
        self._e0.record(self.stream)
        self._t0 = time.perf_counter()

    def end(self):
        e1 = self.torch.cuda.Event(enable_timing=True)
        e1.record(self.stream)
        self.stream.synchronize()
        self.call_ms += max(self._e0.elapsed_time(e1), 1e3 * (time.perf_counter() - self._t0))


class OrderedIO:
    """Everything behind a hold on one stream (see the module docstring).  `stream`: the held
    stream a probe kept; `clobber`: overwrite the host tables given through host() with their
    decoys as soon as a call returns."""
    ordered = True

    def __init__(self, dev, call_ms, what="", stream=None, floor_ms=HOLD_MIN_MS, clobber=False):
        import torch
        self.torch, self.dev, self.what = torch, dev, what
        self.S = stream if stream is not None else torch.cuda.Stream(dev)
        self.setup = torch.cuda.Stream(dev)      # decoy uploads and sentinels: never the null stream
        self.hold_ms = hold_ms_for(call_ms, floor_ms)
        self.call_ms = call_ms
        self.clobber = clobber
        self.keep, self.pending, self.hosts = [], [], []
        self.held = False
        self.calls = 0
        self.returned_early = []                 # per call: the hold was still running on return
        _calibrate(dev)

    def up(self, real, decoy=None):
        torch = self.torch
        real = np.ascontiguousarray(real)
        decoy = real if decoy is None else np.ascontiguousarray(decoy)
        assert decoy.shape == real.shape and decoy.dtype == real.dtype, (self.what, decoy.shape, real.shape)
        with torch.cuda.stream(self.setup):
            d = torch.from_numpy(decoy).to(self.dev)                 # blocking
        pinned = torch.from_numpy(real).pin_memory()
        self.keep += [d, pinned]
        self.pending.append((d, pinned))
        return d

    def put(self, dst, real, decoy=None):
        torch = self.torch
        real = np.ascontiguousarray(real).reshape(tuple(dst.shape))
        decoy = real if decoy is None else np.ascontiguousarray(decoy).reshape(tuple(dst.shape))
        with torch.cuda.stream(self.setup):
            dst.copy_(torch.from_numpy(decoy).to(self.dev))
        self.setup.synchronize()
        pinned = torch.from_numpy(real).pin_memory()
        self.keep += [dst, pinned]
        self.pending.append((dst, pinned))
        return dst

    def full(self, shape, value, dtype):
        with self.torch.cuda.stream(self.setup):
            t = self.torch.full(shape, value, dtype=dtype, device=self.dev)
        self.keep.append(t)
        return t

    def on_stream(self):
        return self.torch.cuda.stream(self.S)

    def host(self, real, decoy=None):
        """A host table of the caller's: a private copy that end() overwrites with the decoy."""
        h = np.array(real, copy=True)
        if decoy is not None:
            decoy = np.asarray(decoy, h.dtype)
            assert decoy.shape == h.shape
            self.hosts.append((h, decoy))
        return h

    @property
    def stream(self):
        return self.S

    @property
    def stream_ptr(self):
        return self.S.cuda_stream

    def begin(self):
        torch = self.torch
        if not self.held:
            torch.cuda.synchronize(self.dev)     # the decoys and sentinels are in place
            enqueue_hold(self.S, self.dev, self.hold_ms)
            self.held = True
        else:
            self.setup.synchronize()
        with torch.cuda.stream(self.S):
            for d, pinned in self.pending:
                d.copy_(pinned, non_blocking=True)
        self.pending = []

    def end(self):
        self.returned_early.append(not self.S.query())
        self.calls += 1
        if self.clobber:
            for h, decoy in self.hosts:
                h[...] = decoy
        self.hosts = []

    def down(self, t):
        if t is None:
            return None
        torch = self.torch
        self.setup.synchronize()
        pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        with torch.cuda.stream(self.S):
            pinned.copy_(t, non_blocking=True)
        self.keep += [t, pinned]
        return pinned.numpy()                    # filled once finish() has returned

    def finish(self, expect_async=True):
        """Synchronise the held stream only.  Every call must have returned while the hold was
        still running: the library did not block, and the run was not vacuous."""
        still_held = not self.S.query()
        self.S.synchronize()
        print(f"{self.what}: synchronous calls {self.call_ms:.3f} ms, hold {self.hold_ms:.0f} ms, {self.calls} call(s), "
              f"returned behind the hold {self.returned_early}, outputs queued behind it {still_held}")
        if expect_async:
            assert all(self.returned_early), (self.what, "a call returned after the hold had run out: it blocked",
                                              self.returned_early)
            assert still_held, (self.what, "the hold ran out before the outputs were queued")


class ProbeIO(OrderedIO):
    """The liveness probe's run: the real uploads wait behind the hold, the call goes to the
    handle's own stream, and the outputs are read after a device synchronise."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.outs = []

    @property
    def stream(self):
        return None

    @property
    def stream_ptr(self):
        return None

    def on_stream(self):
        return self.torch.cuda.stream(self.setup)

    def down(self, t):
        if t is None:
            return None
        a = np.empty(tuple(t.shape), dtype=self.torch.empty(0, dtype=t.dtype).numpy().dtype)
        self.outs.append((a, t))
        return a

    def finish(self, expect_async=True):
        self.S.synchronize()
        self.torch.cuda.synchronize(self.dev)
        for a, t in self.outs:
            a[...] = t.cpu().numpy()


def same_bytes(a, b, what, keys=None):
    """Every output array of two runs byte for byte."""
    for k in (keys if keys is not None else a):
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert x is not None and y is not None, (what, k)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def differs(a, b, keys):
    return any(a[k].tobytes() != b[k].tobytes() for k in keys if isinstance(a[k], np.ndarray))


def probe(dev, run, keys, what, floor_ms=HOLD_MIN_MS):
    """run(io, decoy_only) -> dict of outputs; keys: the outputs that are no input as well (the
    real upload, which comes after the early call, overwrites an in/out buffer).  Returns (held stream, synchronous outputs on
    the real inputs, their GPU time in ms).  Fails when no held stream shows the violation."""
    import torch
    io = SyncIO(dev)
    real = run(io, False)
    call_ms = io.call_ms
    want = run(SyncIO(dev), True)
    assert differs(real, want, keys), (what, "the decoy gives the real problem's outputs")
    for attempt in range(PROBE_STREAMS):
        s = torch.cuda.Stream(dev)
        pio = ProbeIO(dev, call_ms, what + " probe", stream=s, floor_ms=floor_ms)
        got = run(pio, False)
        pio.finish()
        if not differs(got, want, keys):
            print(f"{what}: liveness probe saw the decoy's bytes on held stream {attempt + 1} of {PROBE_STREAMS}")
            return s, real, call_ms
    raise AssertionError(f"{what}: on {PROBE_STREAMS} held streams a call on the handle's own stream was ordered "
                         "behind the hold: a launch on the wrong stream would go unseen")


# ---- decoys ------------------------------------------------------------------------------------
def check_decoy(real: dict, decoy: dict, payload: set, what=""):
    """The decoy rule on two dicts of upload arrays: same keys, shapes and types; arrays named
    in `payload` differ, every other array (indices, offsets, counts) is equal."""
    assert set(real) == set(decoy), what
    seen = set()
    for k, a in real.items():
        b = decoy[k]
        if not isinstance(a, np.ndarray):
            assert (a is None and b is None) or a == b, (what, k)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if k in payload:
            assert a.size and not np.array_equal(a, b), (what, k, "the payload does not differ")
            seen.add(k)
        else:
            assert np.array_equal(a, b), (what, k, "an index array differs")
    assert seen == set(payload), (what, set(payload) - seen)


def decoy_pose_opt(sc):
    """A PoseOptimization frame with the same MapPoint ids, octaves and stereo pattern; keypoints,
    right coordinates, MapPoint positions and the start pose moved."""
    d = dict(sc)
    n = sc["n"]
    d["keys_xy"] = sc["keys_xy"].copy()
    d["keys_xy"][:n] += np.float32([2.5, -1.75])
    if sc["u_right"] is not None:
        d["u_right"] = np.where(sc["u_right"] >= 0, sc["u_right"] + np.float32(2.25), sc["u_right"]).astype(np.float32)
    d["pos"] = (sc["pos"] + np.float32([0.03, -0.02, 0.05])).astype(np.float32)
    d["tcw"] = sc["tcw"].copy()
    d["tcw"][[3, 7, 11]] += np.float32([0.02, 0.01, -0.03])
    return d


def decoy_local_ba(sc):
    """A local map with the same tables of indices; poses, points and keypoints moved."""
    d = dict(sc)
    d["Tcw"] = sc["Tcw"].copy()
    d["Tcw"][:, [3, 7, 11]] += np.float32([0.01, -0.02, 0.015])
    d["pos"] = (sc["pos"] + np.float32([0.02, 0.03, -0.04])).astype(np.float32)
    d["kps_xy"] = (sc["kps_xy"] + np.float32([1.5, -2.25])).astype(np.float32)
    if sc["u_right"] is not None:
        d["u_right"] = np.where(sc["u_right"] >= 0, sc["u_right"] + np.float32(1.25), sc["u_right"]).astype(np.float32)
    return d


def decoy_optimize_sim3(sc):
    """A loop candidate with the same match tables; keypoints, MapPoints, poses and the start moved."""
    d = dict(sc)
    for k, dx in (("k1_xy", [1.25, -0.5]), ("k2_xy", [-0.75, 1.5])):
        d[k] = (sc[k] + np.float32(dx)).astype(np.float32)
    d["mp_pos"] = (sc["mp_pos"] + np.float32([0.02, -0.03, 0.04])).astype(np.float32)
    for k in ("Tcw1", "Tcw2"):
        d[k] = sc[k].copy()
        d[k][[3, 7, 11]] += np.float32([0.01, 0.02, -0.01])
    c, s_ = np.float32(np.cos(0.01)), np.float32(np.sin(0.01))
    Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]], np.float32)
    d["R12"] = (Rz @ np.asarray(sc["R12"], np.float32).reshape(3, 3)).reshape(9).astype(np.float32)
    d["t12"] = (np.asarray(sc["t12"], np.float32) + np.float32([0.01, -0.01, 0.02])).astype(np.float32)
    d["s12"] = np.float32(sc["s12"]) * np.float32(1.01)
    return d


def decoy_essential_graph(sc):
    """A pose graph with the same edges; poses, corrected Sim3s (translation) and points moved."""
    d = dict(sc)
    d["Tcw"] = np.array(sc["Tcw"], np.float32, copy=True).reshape(-1, 12)
    d["Tcw"][:, [3, 7, 11]] += np.float32([0.03, -0.02, 0.01])
    d["Tcw"] = d["Tcw"].reshape(np.asarray(sc["Tcw"]).shape)
    d["corr_S"] = np.array(sc["corr_S"], np.float64, copy=True)
    d["corr_S"][:, 4:7] += [0.02, 0.01, -0.03]
    d["pos"] = (np.asarray(sc["pos"], np.float32) + np.float32([0.05, 0.02, -0.04])).astype(np.float32)
    return d


def decoy_covisibility(kf_mp, kf_n, kf_bad, mp_bad, seed=77):
    """Another valid all-integer table of the same id range: every keyframe loses some of its
    points and gains others of the range; other bad points."""
    rng = np.random.default_rng(seed)
    out = np.array(kf_mp, np.int32, copy=True)
    n = len(mp_bad)
    for k in range(len(out)):
        have = np.flatnonzero(out[k] >= 0)
        out[k, rng.permutation(have)[:max(1, len(have) // 3)]] = -1
        free = np.flatnonzero(out[k] < 0)
        out[k, rng.permutation(free)[:6]] = rng.integers(0, n, min(6, len(free)))
    bad = np.zeros_like(mp_bad)
    bad[rng.permutation(n)[:int(mp_bad.sum()) + 3]] = 1
    return out, np.array(kf_n, copy=True), np.array(kf_bad, copy=True), bad


def decoy_bows(bows, seed=78):
    """BowVectors with the same words and other values (L1-normalised again)."""
    rng = np.random.default_rng(seed)
    out = []
    for b in bows:
        v = {w: x * float(rng.uniform(0.5, 1.5)) for w, x in b.items()}
        s = sum(v.values())
        out.append({w: x / s for w, x in v.items()} if len(v) > 1 else {w: 0.5 * x for w, x in v.items()})
    return out
