"""The stream contract on the GPU: every op of tests/stream_cases.py on a side stream while the default stream is busy.

INTEGRATION.md promises "thread-safe per stream; no global state in the library", and every entry point takes a stream.
The rest of the suite calls everything on the default stream (handle 0), where a launch that dropped its stream argument,
a handle remembered from construction or a cached device tensor built on another stream all behave as if they were right.

The method: finite GPU work of a known duration (`busy`, torch.cuda._sleep in 5 ms pieces) is queued on the DEFAULT stream
and an event is recorded behind it; the case then runs under a side stream and its results are fetched by copies on that
stream alone.  Whatever went to the default stream by mistake — a kernel, a fill, a copy — is still queued behind the delay
when its consumer on the side stream runs, so the consumer reads memory that was never written: the comparison with the
idle-stream reference fails.  A run only counts if the event behind the delay has NOT completed when the last result has
been fetched (otherwise it proves nothing, and the test fails rather than passing for no reason).
Before every measured run the free memory of torch's allocator and the pooled arenas are filled with 0xFF bytes
(poison_free_memory): a buffer that was never written must not still hold the right answer of the run before.

(a) every case of the table, (b) the symbols a case claims are really called (a recording wrapper on the ctypes object),
(c) objects that used to remember the stream of their construction, (d) two frames interleaved on two streams from one host
thread, (e) the fallback branch of the polled read-back (a stream with more queued work than kPollTimeoutUs),
(f) the cached band table of rolling-shutter frames across streams.  Numbers: profiles/stream_tests.md.

Comparison: bitwise (two runs of the reference are compared first to confirm that the case is bit-reproducible) except for
the outputs listed in TOLERANCED, which accumulate with float atomics; those take the bound of their family's own test.
At most two side streams are used; with the default stream and the one stream the binding owns for blocking uploads
(ops._upload_blocking) a process of (d) or (f) holds four, the number of hardware queues the machines give a process."""
import ctypes
import json
import math
import os
import re
import time
from pathlib import Path

import pytest
import torch

import stream_cases as C

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
POLL_TIMEOUT_US = int(re.search(r"constexpr long long kPollTimeoutUs = (\d+);",
                                (ROOT / "3dgs-deblur_amd" / "csrc" / "frame.hip").read_text()).group(1))
MIN_DELAY_MS = 40.0

# outputs that are NOT bit-reproducible from run to run, with the bound their family's own GPU test holds them to: the
# gsplat-compatible rasterize_gaussians has no emission index, so gs_rasterize_bwd accumulates the per-Gaussian gradients
# with fp32 atomics (csrc/raster_bwd.hip, OUT = 0); tests/test_gpu_parity.py::test_rasterize_gaussians_parity holds them to
# GRAD_RTOL = 3e-3 of the tensor's largest |g|.  Everything else, these outputs' forward values included, is bitwise.
TOLERANCED = {"rasterize_gaussians": {k: 3e-3 for k in ("grad_xys", "grad_conics", "grad_colors", "grad_opacity")}}

REPORT = {}


# ---- the delay ----------------------------------------------------------------------------------------------------------------
class Delay:
    """busy(stream, ms): queue GPU work of at least `ms` milliseconds on `stream`.  It ends by construction: pieces of
    torch.cuda._sleep (a kernel that spins for a fixed number of clock cycles), or — a torch build without it — a chain of
    elementwise ops on a scratch tensor; nothing waits on a flag or on host memory.  Calibrated once on an idle device."""
    PIECE_MS = 5.0

    def __init__(self, dev):
        self.dev = dev
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.scratch = None if self.sleep is not None else torch.ones(1 << 24, device=dev)
        self.units = 1_000_000 if self.sleep is not None else 4
        for _ in range(3):                      # the first measurement carries first-launch effects
            t = self._measure()
            self.units = max(1, int(self.units * self.PIECE_MS / max(t, 1e-3)))
        self.piece_ms = self._measure()
        assert 0.25 * self.PIECE_MS < self.piece_ms < 4 * self.PIECE_MS, self.piece_ms

    def _piece(self):
        if self.sleep is not None:
            self.sleep(self.units)
        else:
            for _ in range(self.units):
                self.scratch.mul_(1.0)

    def _measure(self):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self._piece()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def busy(self, stream, ms):
        with torch.cuda.stream(stream):
            for _ in range(int(math.ceil(1.25 * ms / self.piece_ms))):       # a quarter more than asked: never less
                self._piece()


@pytest.fixture(scope="module")
def delay(dev):
    return Delay(dev)


@pytest.fixture(scope="module")
def streams(dev):
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


@pytest.fixture(scope="module", autouse=True)
def report_file():
    """GSD_STREAM_REPORT=<path>: the per-case figures of this run as JSON (how profiles/stream_tests.md was made)"""
    yield
    path = os.environ.get("GSD_STREAM_REPORT")
    if path and REPORT:
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text(json.dumps(REPORT, indent=1, sort_keys=True))


# ---- the recording wrapper ----------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []                 # (symbol, host seconds inside the call)

    def wrap(self, name, real):
        def call(*args):
            t0 = time.perf_counter()
            try:
                return real(*args)
            finally:
                self.calls.append((name, time.perf_counter() - t0))
        return call

    def clear(self):
        self.calls = []

    def names(self):
        return {n for n, _ in self.calls}


@pytest.fixture
def recorder(gs, monkeypatch):
    """every entry point of the loaded library behind a wrapper that notes the call and calls straight through"""
    lib, rec = gs._lib.load(), Recorder()
    for name in gs._lib._SIGS:
        monkeypatch.setattr(lib, name, rec.wrap(name, getattr(lib, name)))
    return rec


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def fetch(res):
    """the results on the host, by copies on the CURRENT stream (each waits for that stream alone)"""
    return {k: v.detach().cpu() for k, v in res.items()}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.contiguous().numpy().tobytes() == b.contiguous().numpy().tobytes()


def differing(a, b):
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    return sorted(k for k in a if not same_bits(a[k], b[k]))


def assert_matches(name, got, ref):
    tol = TOLERANCED.get(name, {})
    bad = [k for k in differing(got, ref) if k not in tol]
    assert not bad, f"{name}: differs from the idle-stream reference in {bad}"
    for k, bound in tol.items():
        err = float((got[k].double() - ref[k].double()).abs().max() / ref[k].double().abs().max())
        assert err <= bound, (name, k, err, bound)


def poison_free_memory(dev, streams):
    """Make stale memory WRONG before a measured run.  The run reuses the memory of the runs before it: torch's allocator
    hands the same cached blocks to the same sequence of allocations, so a buffer that a misdirected launch never wrote
    would still hold the right answer of the warm-up run and the comparison would pass (profiles/stream_tests.md).  Every
    free cached block of the allocator (default stream, side streams, the binding's upload stream) and every pooled frame
    arena is filled with 0xFF bytes (a NaN as a float, -1 as an integer); the pooled gradient buffers, which hold the last
    run's gradients by design, are dropped.  A correct library never reads memory it has not written."""
    from gsdeblur_amd import ops
    torch.cuda.synchronize()
    with ops._state_lock:
        ops._grad_pool.clear()
        arenas = [a.tensor if hasattr(a, "tensor") else a for pool in ops._arena_pool.values() for a in pool]
    for t in arenas:
        t.fill_(0xFF)
    by_handle = {st.cuda_stream: st for st in (torch.cuda.default_stream(dev),) + tuple(streams)
                 + tuple(ops._upload_streams.values())}
    held = []
    for _ in range(16):                         # blocks larger than a request of their pool are taken in pieces
        todo = []
        for seg in torch.cuda.memory_snapshot():
            st = by_handle.get(seg["stream"])
            if seg["device"] != dev.index or st is None:
                continue
            cap = (1 << 20) if seg["segment_type"] == "small" else None          # requests above 1 MiB leave the small pool
            todo += [(st, b["size"] if cap is None else min(b["size"], cap)) for b in seg["blocks"] if b["state"] == "inactive"]
        if not todo:
            break
        for st, size in sorted(todo, key=lambda x: -x[1]):
            with torch.cuda.stream(st):
                t = torch.empty(size, dtype=torch.uint8, device=dev)
                t.fill_(0xFF)
            held.append(t)
    torch.cuda.synchronize()
    # every call follows runs that freed memory: if nothing was found, the snapshot's layout (segment_type, blocks[].state,
    # stream) is no longer what this function reads and the poisoning has silently stopped
    assert held, "poison_free_memory found no free cached block: torch.cuda.memory_snapshot() no longer reads as expected"
    del held
    torch.cuda.synchronize()


def run_behind_busy_default(dev, delay, s, ms, fn):
    """queue `ms` of work on the default stream, run fn() under s, fetch under s -> (results, delay still running?)"""
    default = torch.cuda.default_stream(dev)
    ev = torch.cuda.Event()
    delay.busy(default, ms)
    ev.record(default)
    with torch.cuda.stream(s):
        got = fetch(fn())
        still_busy = not ev.query()
    return got, still_busy


# ---- (a) + (b): every case on a side stream, default stream busy --------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_case_on_a_side_stream_while_the_default_stream_is_busy(gs, dev, streams, delay, recorder, case):
    s = streams[0]
    with torch.cuda.stream(s):                  # warm-up where the case will run: allocator pool, pinned buffers, arenas
        fetch(case.run(gs, dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = fetch(case.run(gs, dev))              # idle default stream
    wall_ms = (time.perf_counter() - t0) * 1e3
    again = fetch(case.run(gs, dev))
    torch.cuda.synchronize()
    unstable = differing(ref, again)
    assert set(unstable) <= set(TOLERANCED.get(case.name, {})), f"not bit-reproducible on an idle stream: {unstable}"
    d_ms = max(4.0 * wall_ms, MIN_DELAY_MS)
    poison_free_memory(dev, streams)
    recorder.clear()
    try:
        got, still_busy = run_behind_busy_default(dev, delay, s, d_ms, lambda: case.run(gs, dev))
        called = recorder.names()
        REPORT[case.name] = dict(wall_ms=round(wall_ms, 2), delay_ms=round(d_ms, 1), valid=bool(still_busy),
                                 comparison="toleranced: " + ", ".join(TOLERANCED[case.name]) if case.name in TOLERANCED
                                 else "bitwise", also_called=sorted(called - set(case.covers)))
        print(f"{case.name}: wall {wall_ms:.2f} ms, delay {d_ms:.1f} ms, valid {still_busy}, "
              f"called beyond covers {sorted(called - set(case.covers))}")
        assert still_busy, "the delay on the default stream had ended before the results were fetched: the run proves nothing"
        assert_matches(case.name, got, ref)
        assert set(case.covers) <= called, f"never called: {sorted(set(case.covers) - called)}"
    finally:
        torch.cuda.synchronize()


# ---- (c): objects that are built under one stream and used under another ------------------------------------------------------
def test_dp_row_ops_built_on_the_default_stream_follow_the_callers_stream(gs, dev, streams, delay, recorder):
    """dp._RowOps used to remember the stream current at construction; its buffers are torch allocations on the CALLER's
    stream, so it now takes the stream current at each call (dp.py)."""
    from gsdeblur_amd.dp import _RowOps
    s = streams[0]

    def build():
        return _RowOps(C.dp_grads(dev)), _RowOps([torch.zeros(sh, device=dev) for sh in C.DP_SHAPES])
    ref = fetch(C.dp_exchange(*build()))
    rows, acc = build()                          # built under the default stream ...
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert rows._stream.value == s.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
        fetch(C.dp_exchange(*build()))           # warm-up of the side stream's allocator pool
    poison_free_memory(dev, streams)
    try:
        got, still_busy = run_behind_busy_default(dev, delay, s, MIN_DELAY_MS, lambda: C.dp_exchange(rows, acc))   # ... used under s
        assert still_busy
        assert not differing(got, ref)
        assert set(C.by_name("dp_rows").covers) <= recorder.names()
    finally:
        torch.cuda.synchronize()


def test_mesh_clean_run_built_on_the_default_stream_follows_the_callers_stream(gs, dev, streams, delay):
    """meshclean._Run likewise: its launches go to the stream current at each launch."""
    M = gs.meshclean
    s = streams[0]
    V, verts, faces, colors = C.mesh_inputs(dev)
    ref = fetch(dict(zip(("labels", "roots", "face_counts", "vert_counts"), gs.mesh_components(faces, V, return_table=True))))
    run = M._Run(faces, V, "mesh_components")                           # built under the default stream
    n_comp = run.read_counts()[M.COMPONENTS]
    with torch.cuda.stream(s):
        fetch(dict(zip("abcd", gs.mesh_components(faces, V, return_table=True))))          # warm-up of the side stream
    poison_free_memory(dev, streams)
    vp = ctypes.c_void_p

    def table():
        assert run.stream.value == s.cuda_stream
        outs = [torch.full((n_comp,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
        run.check(run.lib.gs_mesh_components_table(V, run.F, n_comp, *(vp(t.data_ptr()) for t in outs), run.p_ws, run.ws_bytes,
                                                   run.stream), "mesh_components table")
        return dict(zip(("roots", "face_counts", "vert_counts"), outs), labels=run.labels)
    try:
        got, still_busy = run_behind_busy_default(dev, delay, s, MIN_DELAY_MS, table)
        assert still_busy
        assert not differing(got, ref)
    finally:
        torch.cuda.synchronize()


# ---- the recycled gradient buffer behind the delay -------------------------------------------------------------------------
def test_recycled_gradient_buffer_behind_the_delay(gs, dev, streams, delay):
    """poison_free_memory drops the pooled gradient buffers, so the cases above only run the fresh form of
    gs_project_fused_bwd_pooled (full fill) behind the delay.  Here two frames of one scene run behind ONE delay, the
    second with other loss weights: it recycles the first's buffer (only the dirty rows are zeroed), and what that buffer
    still holds — the first frame's gradients — is not the second's answer."""
    from gsdeblur_amd import ops
    s = streams[0]
    prep = C.rc_prepare(gs, dev)
    prep2 = dict(prep, wc=prep["wc"] * -0.7, wd=prep["wd"] * 1.3, wa=prep["wa"] * -0.4)
    key = (str(dev), s.cuda_stream)
    entries = []

    def two_frames():
        out = []
        for p in (prep, prep2):
            st = C.rc_forward(gs, p)
            res = C.rc_backward(st)
            out.append(fetch(res))
            del st, res                          # nothing outside the pool reaches the buffer any more: it may be recycled
            entries.append([id(e) for e in ops._grad_pool.get((str(dev), torch.cuda.current_stream().cuda_stream), [])])
        return out
    ref = two_frames()
    assert differing(ref[0], ref[1])
    with torch.cuda.stream(s):
        two_frames()
    torch.cuda.synchronize()
    poison_free_memory(dev, streams)
    del entries[:]
    default = torch.cuda.default_stream(dev)
    ev = torch.cuda.Event()
    try:
        delay.busy(default, 2 * MIN_DELAY_MS)
        ev.record(default)
        with torch.cuda.stream(s):
            got = two_frames()
            still_busy = not ev.query()
        assert still_busy, "the delay on the default stream had ended before the results were fetched"
        assert len(entries[0]) == 1 and entries[1] == entries[0], (entries, sorted(ops._grad_pool), key)   # recycled
        assert not differing(got[0], ref[0])
        assert not differing(got[1], ref[1])
    finally:
        torch.cuda.synchronize()


# ---- (d): two frames interleaved on two streams ---------------------------------------------------------------------------------
def test_two_frames_interleaved_on_two_streams(gs, dev, streams, delay):
    """forward A on s1, forward B on s2, backward B, backward A from one host thread, the default stream busy throughout:
    every image and gradient equals the scene rendered alone, and the arenas and gradient buffers of the two frames live in
    the pools of their own streams."""
    from gsdeblur_amd import ops
    s1, s2 = streams
    prep = {"A": C.rc_prepare(gs, dev, seed=41), "B": C.rc_prepare(gs, dev, seed=43)}
    alone = {k: fetch(C.rc_backward(C.rc_forward(gs, p))) for k, p in prep.items()}
    assert differing(alone["A"], alone["B"])                   # two scenes of one shape with different values
    for s in (s1, s2):                                         # warm-up of both streams' allocator pools
        with torch.cuda.stream(s):
            fetch(C.rc_backward(C.rc_forward(gs, prep["A"])))
    torch.cuda.synchronize()
    ops.release_arenas()
    poison_free_memory(dev, streams)
    default = torch.cuda.default_stream(dev)
    ev = torch.cuda.Event()
    try:
        delay.busy(default, 6 * MIN_DELAY_MS)
        ev.record(default)
        with torch.cuda.stream(s1):
            st_a = C.rc_forward(gs, prep["A"])
        with torch.cuda.stream(s2):
            st_b = C.rc_forward(gs, prep["B"])
            res_b = C.rc_backward(st_b)
        with torch.cuda.stream(s1):
            res_a = C.rc_backward(st_a)
            got_a = fetch(res_a)
        with torch.cuda.stream(s2):
            got_b = fetch(res_b)
        assert not ev.query(), "the delay on the default stream had ended before the results were fetched"
        assert not differing(got_a, alone["A"])
        assert not differing(got_b, alone["B"])
        del st_a, st_b, res_a, res_b                           # the frames' autograd nodes hand their arenas back
        keys = {k: (str(dev), s.cuda_stream) for k, s in (("s1", s1), ("s2", s2), ("default", default))}
        assert len({keys["s1"], keys["s2"], keys["default"]}) == 3
        for pool in (ops._arena_pool, ops._grad_pool):
            assert pool.get(keys["s1"]) and pool.get(keys["s2"]), sorted(pool)
            assert not pool.get(keys["default"]), sorted(pool)
        a1, a2 = ops._arena_pool[keys["s1"]], ops._arena_pool[keys["s2"]]
        assert not {x.data_ptr() for x in a1} & {x.data_ptr() for x in a2}
    finally:
        torch.cuda.synchronize()


# ---- (e): the polled read-back under backlog ----------------------------------------------------------------------------------
def test_polled_read_back_behind_a_backlog(gs, dev, streams, delay, recorder):
    """gs_frame_forward polls a pinned sequence word for its read-backs and falls back to a stream synchronisation after
    kPollTimeoutUs (csrc/frame.hip read_back) — the state of a trainer whose host runs ahead of the GPU.  The frame's own
    stream holds 1.5 x the timeout of queued work, and the frame's inputs are copied into place behind it (until then the
    buffers hold another valid scene of the same shape: a launch that ran early would give a wrong picture, never a wild
    index).  Both read-back modes must give the idle-stream result, and the polled forward must have waited out the timeout."""
    from gsdeblur_amd import ops
    s = streams[0]
    timeout_ms = POLL_TIMEOUT_US / 1e3
    prep, stale = C.rc_prepare(gs, dev, seed=41), C.rc_prepare(gs, dev, seed=43)
    ref = fetch(C.rc_backward(C.rc_forward(gs, prep)))
    with torch.cuda.stream(s):                                 # warm-up: the pinned buffer and the arena of this stream
        fetch(C.rc_backward(C.rc_forward(gs, prep)))
    torch.cuda.synchronize()
    old = ops.FRAME_POLL
    try:
        for poll in (1, 0):
            ops.FRAME_POLL = poll
            buf = {k: v.clone() for k, v in stale["params"].items()}
            poison_free_memory(dev, streams)
            recorder.clear()
            with torch.cuda.stream(s):
                if poll:
                    assert ops.frame_poll() == 1
                delay.busy(s, 1.5 * timeout_ms)
                # nothing from here to gs_frame_forward may block the host (every cache it passes — _band_edges,
                # _band_tile_done, the pinned buffer, the arena — is warm from the warm-up): the wait below is the frame's own
                for k, v in prep["params"].items():
                    buf[k].copy_(v)                            # right only behind the delay
                st = C.rc_forward(gs, prep, leaves=buf)
                got = fetch(C.rc_backward(st))
            fwd_ms = max(t for n, t in recorder.calls if n == "gs_frame_forward") * 1e3
            REPORT[f"backlog_poll{poll}"] = dict(frame_forward_ms=round(fwd_ms, 1), timeout_ms=timeout_ms)
            print(f"backlog, FRAME_POLL={poll}: the gs_frame_forward call took {fwd_ms:.1f} ms of host time "
                  f"(kPollTimeoutUs = {timeout_ms:.0f} ms)")
            assert not differing(got, ref), f"FRAME_POLL={poll}"
            if poll:
                assert fwd_ms >= timeout_ms, "the polled read-back returned before its timeout: the fallback did not run"
    finally:
        ops.FRAME_POLL = old
        torch.cuda.synchronize()


# ---- (f): a cached device tensor across streams -------------------------------------------------------------------------------
def _band_frame(gs, dev, prm, times, H, W, S, R, sc):
    from gsdeblur_amd import ops
    vms = gs.subpose_viewmats(prm["viewmat"], prm["lin_vel"], prm["ang_vel"], times)
    with torch.no_grad():
        rgb, al, radii = gs.render_combined(prm["means"], prm["log_scales"].exp(), prm["quats"],
                                            torch.sigmoid(prm["opacity_logits"]), prm["sh"], vms, None, S, R, sc["fx"],
                                            sc["fy"], sc["cx"], sc["cy"], H, W, gamma=2.2, min_rgb_level=10.0,
                                            sh_degree=sc["deg"], hints=ops.FrameHints())
    return dict(rgb=rgb, alphas=al, radii=radii)


def test_cached_band_table_is_complete_for_a_second_stream(gs, dev, streams, delay):
    """ops._band_tile_done caches the initial tile_done of a rolling-shutter frame per shape, for every stream.  The table
    of a new shape is asked for under s1 behind a delay — the call alone, no frame: a whole frame on s1 reads back from the
    device and so waits for everything queued there, its own table included — and a frame of that shape runs at once on s2.
    Valid only if the delay on s1 is still running when the frame's results have been fetched.  The table must be complete
    by then: it is uploaded by a blocking copy on the binding's own stream.  Built by device ops on the current stream it
    would still be queued behind the delay, s2 would read a table of 0xFF bytes (every tile done) and the image would be the
    background."""
    from gsdeblur_amd import ops
    s1, s2 = streams
    W, H, S, R = 64, 80, 3, 2                                  # 4 x 5 tiles: a shape no other test uses
    sc = C._scene(gs, 400, W, H, seed=47)
    prm = {k: sc[k].float().to(dev) for k in C.G_NAMES + C.CAM_NAMES}
    times = torch.tensor(gs.subpose_schedule(S, 1 / 60, R, 1 / 30)[0], device=dev)
    ref = fetch(_band_frame(gs, dev, prm, times, H, W, S, R, sc))
    assert float(ref["rgb"].max()) > 0
    for s in (s2, s1):                                         # warm-up: s2 is where the frame will run; s1's allocator pool
        with torch.cuda.stream(s):                             # must hold (poisoned) blocks for a table built there, not
            fetch(_band_frame(gs, dev, prm, times, H, W, S, R, sc))       # fresh memory.  _band_edges stays warm
            torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ty, tx = (H + 15) // 16, (W + 15) // 16
    key = (S, R, ty, tx, str(prm["means"].device))
    assert key in ops._band_done_cache
    ops._band_done_cache.clear()
    poison_free_memory(dev, streams)
    ev = torch.cuda.Event()
    try:
        delay.busy(s1, 1.5 * MIN_DELAY_MS)
        ev.record(s1)
        with torch.cuda.stream(s1):
            table = ops._band_tile_done(S, R, ty, tx, prm["means"].device)
        assert ops._band_done_cache.get(key) is table
        with torch.cuda.stream(s2):
            second = fetch(_band_frame(gs, dev, prm, times, H, W, S, R, sc))
            still_busy = not ev.query()
        assert still_busy, "the delay on s1 had ended before the frame on s2 was fetched: the run proves nothing"
        assert ops._band_done_cache.get(key) is table          # the frame took the cached table
        assert not differing(second, ref)
    finally:
        torch.cuda.synchronize()
