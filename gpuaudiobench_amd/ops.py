"""Kernel- and plan-level calls of the C ABI on torch device tensors.

Every function forwards raw device pointers and the current torch stream to
libgab_hip.so; outputs are allocated with torch (device memory plumbing only).
Argument names and meaning follow the reference kernels (see gab_c_api.h).
"""
import ctypes as C

import torch

from ._capi import (lib, check, WaveguideState, FdtdParams, CONV_STATELESS, CONV_STREAMING,
                    CONV_STREAMING_HOST_IO,
                    DWG_NAIVE, DWG_ACCEL)


def _stream(stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def _dev(t, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("expected a CUDA/HIP tensor")
    if t.dtype != dtype:
        raise TypeError("expected dtype %s, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _acc(t, dtype=torch.float32):
    """Device-ACCESSIBLE memory: a device tensor, or a pinned host tensor (hipHostMalloc memory is
    mapped into the device's address space, so a kernel can read and write it over PCIe)."""
    if isinstance(t, torch.Tensor) and not t.is_cuda and t.is_pinned():
        if t.dtype != dtype:
            raise TypeError("expected dtype %s, got %s" % (dtype, t.dtype))
        if not t.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return C.c_void_p(t.data_ptr())
    return _dev(t, dtype)


def _view(ptr, rows, cols):
    """A torch tensor over library-owned device memory (no ownership: keep the plan alive)."""
    class _Mem:
        pass
    m = _Mem()
    m.__cuda_array_interface__ = {"shape": (rows, cols), "typestr": "<f4", "data": (ptr, False), "version": 2}
    return torch.as_tensor(m, device="cuda")


class _Handle:
    """A library object behind a handle `_h`: close() destroys it once, garbage collection closes what was left open."""

    _h = None
    _destroy = None     # the name of its gab_*_destroy

    def close(self):
        if self._h:
            getattr(lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _launcher(name):
    """launch(args) for the tuple a prepare() built: the call of process() without building its arguments again."""
    fn = getattr(lib, name)

    def launch(args):
        check(fn(*args))
    return staticmethod(launch)


class _Prepared:
    """prepare() of a plan whose process call takes (plan, in, out, stream)."""

    def prepare(self, x, out, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers; `launch(args)`."""
        return (self._h, _dev(x), _dev(out), _stream(stream))


def _n_buffers(plan, xs):
    """How many whole buffers of the plan xs holds."""
    n, rest = divmod(xs.numel(), plan.tracks * plan.bufsize)
    assert rest == 0
    return n


def _positions(ptr, n):
    """A copy of a library-owned vector [n] of uint32 positions, as int64."""
    return _view(ptr, n, 1).clone().view(torch.int32).to(torch.int64).view(n)


class _TrackPlan(_Handle):
    """What the track plans (eq, mix, delay, meter, resample, dynamics, reverb, gate, crossover, limiter, spectrum, resynthesis, denoise, saturator, nlms, fdaf, mconv) share: `tracks` channels of
    `bufsize` samples a buffer behind the functions gab_<plan>_* (the prefix is `_destroy`'s)."""

    def _fn(self, what):
        return getattr(lib, self._destroy[:-len("destroy")] + what)

    def _create(self, tracks, bufsize, *rest):
        self.tracks, self.bufsize = tracks, bufsize
        self._h = C.c_void_p()
        check(self._fn("create")(C.byref(self._h), tracks, bufsize, *rest))

    def reset(self):
        check(self._fn("reset")(self._h, _stream()))

    def _rows(self, t, width, first_track, what="table"):
        """How many rows of `width` values t holds: whole rows, and without a first_track one per track."""
        n, rest = divmod(t.numel(), width)
        if rest or n == 0:
            raise ValueError("%s must hold whole rows of %d values" % (what, width))
        if first_track is None and n != self.tracks:
            raise ValueError("%s must hold a row per track (or give first_track)" % what)
        return n

    def _set(self, what, ptr, first_track, n_tracks, *rest):
        """gab_<plan>_set_<what> (first_track None: every track of the plan), else gab_<plan>_set_<what>_tracks."""
        if first_track is None:
            check(self._fn("set_" + what)(self._h, ptr, *rest, _stream()))
        else:
            check(self._fn("set_" + what + "_tracks")(self._h, ptr, first_track, n_tracks, *rest, _stream()))

    def _tables(self, what, width):
        """Copies of (current, target) of the ramped table behind gab_<plan>_<what>, each [tracks][width]."""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        check(self._fn(what)(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return _view(a.value, self.tracks, width).clone(), _view(b.value, self.tracks, width).clone()

    def _process(self, what, xs, out, n, shape, *rest, sized=True):
        """gab_<plan>_<what>(plan, xs, out, *rest, stream) on the n buffers of xs; returns out.  out=None: a new tensor
        of `shape` (None: like xs); a given out holds as many elements (sized=False: not looked at)."""
        assert xs.numel() == n * self.tracks * self.bufsize
        if out is None:
            out = torch.empty_like(xs) if shape is None else torch.empty(shape, dtype=torch.float32, device=xs.device)
        assert not sized or out.numel() == (xs.numel() if shape is None else torch.Size(shape).numel())
        check(self._fn(what)(self._h, _dev(xs), _dev(out), *rest, _stream()))
        return out


class _KeyedPlan(_TrackPlan):
    """The plans with a side chain, dynamics and gate: rows of len(FIELDS) parameters per track, tracks [g link,
    (g + 1) link) on one detector, and a process call of the form (x, key, out, extra): key is what the detector reads
    instead of x, extra an optional block of dtype `_extra` with a word per track and buffer."""

    _extra = torch.float32

    def __init__(self, tracks, bufsize, link=1):
        self.link = link
        self._create(tracks, bufsize, link)

    def set_params(self, table, ramp=True, first_track=None):
        """table: device tensor [tracks][len(FIELDS)], or [n][len(FIELDS)] for tracks [first_track, first_track + n).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        n = self._rows(table, len(self.FIELDS), first_track)
        self._set("params", _dev(table), first_track, n, 1 if ramp else 0)

    def _run(self, what, x, key, out, extra, n):
        """n None: process, one buffer; else process_batch on n buffers."""
        assert n is not None or x.numel() == self.tracks * self.bufsize
        out = torch.empty_like(x) if out is None else out
        assert out.numel() == x.numel() and (key is None or key.numel() == x.numel())
        assert extra is None or extra.numel() == (n or 1) * self.tracks
        rest = () if n is None else (n,)
        check(self._fn(what)(self._h, _dev(x), None if key is None else _dev(key), _dev(out),
                             None if extra is None else _dev(extra, self._extra), *rest, _stream()))
        return out

    def params(self):
        """Copies of (current, target), each [tracks][len(FIELDS)]."""
        return self._tables("params", len(self.FIELDS))


def device_count():
    n = C.c_int(0)
    check(lib.gab_device_count(C.byref(n)))
    return n.value


def noop(x, out=None):
    out = torch.empty_like(x) if out is None else out
    check(lib.gab_noop(_dev(x), _dev(out), x.numel(), _stream()))
    return out


def gain(x, g=2.0, out=None):
    out = torch.empty_like(x) if out is None else out
    check(lib.gab_gain(_dev(x), _dev(out), x.numel(), g, _stream()))
    return out


def gainstats(x, tracks, bufsize, g=0.5):
    out = torch.empty_like(x)
    stats = torch.empty(2 * tracks, dtype=torch.float32, device=x.device)
    check(lib.gab_gainstats(_dev(x), _dev(out), _dev(stats), tracks, bufsize, g, _stream()))
    return out, stats


def datatransfer(x, out_size):
    out = torch.empty(out_size, dtype=torch.float32, device=x.device)
    check(lib.gab_datatransfer(_dev(x) if x.numel() else None, _dev(out) if out_size else None,
                               x.numel(), out_size, _stream()))
    return out


def _placement(fn, handle):
    import numpy as np
    cap = 256
    hw, xc = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    n = C.c_int(0)
    check(fn(handle, hw.ctypes.data_as(C.c_void_p), xc.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    return [dict(xcc=int(x & 0xf), se=int((h >> 13) & 7), sa=int((h >> 12) & 1), cu=int((h >> 8) & 0xf),
                 simd=int((h >> 4) & 3), slot=int(h & 0xf)) for h, x in zip(hw[:n.value], xc[:n.value])]


def placement_summary(places):
    """'8 waves on 8 XCDs: x0/se1/cu3 ...' — one line for a measurement's record."""
    if not places:
        return "no wave has started"
    return "%d waves on %d XCDs: %s" % (len(places), len({p["xcc"] for p in places}),
                                        " ".join("x%d/se%d/cu%d" % (p["xcc"], p["se"], p["cu"]) for p in places[:16]) +
                                        (" ..." if len(places) > 16 else ""))


class KeepWarm(_Handle):
    """gab_keep_warm: a small resident launch that keeps the device from going idle between real-time slots
    (kick() once per slot; it ends by itself idle_seconds after the last kick)."""

    _destroy = "gab_keep_warm_destroy"

    def __init__(self, workgroups=8, idle_seconds=0.25):
        h = C.c_void_p()
        check(lib.gab_keep_warm_create(C.byref(h), int(workgroups), float(idle_seconds)))
        self._h = h

    def kick(self):
        check(lib.gab_keep_warm_kick(self._h))

    def running(self):
        v = C.c_int(0)
        check(lib.gab_keep_warm_running(self._h, C.byref(v)))
        return bool(v.value)

    def placement(self):
        """Where the waves of the current (or last) launch landed: a list of dicts (xcc, se, sa, cu, simd, slot) for every
        wave that has started (gab_keep_warm_placement; HW_ID / XCC_ID as the hardware reports them)."""
        return _placement(lib.gab_keep_warm_placement, self._h)


class LinkPlan(_Handle):
    """gab_link_plan: the staging buffer, words and upload stream of datatransfer with both link directions
    busy at once (gab_datatransfer_round_trip)."""

    _destroy = "gab_link_plan_destroy"

    def __init__(self, max_in_size):
        h = C.c_void_p()
        check(lib.gab_link_plan_create(int(max_in_size), C.byref(h)))
        self._h, self.max_in_size = h, int(max_in_size)

    def round_trip(self, h_in, h_out, stream=None):
        """Pinned host tensor in -> pinned host tensor out; returns when h_out is complete and h_in uploaded."""
        if h_in.is_cuda or h_out.is_cuda or (h_out.numel() and not h_out.is_pinned()):
            raise TypeError("round_trip takes host tensors; the output must be pinned")
        if h_in.dtype != torch.float32 or h_out.dtype != torch.float32 or not h_in.is_contiguous() or not h_out.is_contiguous():
            raise TypeError("round_trip takes contiguous float32 tensors")
        st = _stream(stream)
        check(lib.gab_datatransfer_round_trip(self._h, C.c_void_p(h_in.data_ptr()) if h_in.numel() else None,
                                              C.c_void_p(h_out.data_ptr()) if h_out.numel() else None,
                                              h_in.numel(), h_out.numel(), st))
        return h_out

    def check(self):
        """The verdict of the check launch behind the last round trip (gab_datatransfer_round_trip_check)."""
        check(lib.gab_datatransfer_round_trip_check(self._h))


def iir(x, coeffs, state, tracks, bufsize, sequential=False):
    """state (tracks*2, device) is updated in place.  sequential=True forces the
    lane-per-track kernel that is bit-identical to the golden."""
    out = torch.empty_like(x)
    c = (C.c_float * 5)(*[float(v) for v in coeffs])
    fn = lib.gab_iir_sequential if sequential else lib.gab_iir
    check(fn(_dev(x), _dev(out), c, _dev(state), tracks, bufsize, _stream()))
    return out


def conv1d(x, ir, ir_len, tracks, bufsize):
    out = torch.empty(tracks * bufsize, dtype=torch.float32, device=x.device)
    check(lib.gab_conv1d(_dev(x), _dev(out), _dev(ir), ir_len, tracks, bufsize, _stream()))
    return out


def rndmem(pool, playheads, tracks, bufsize):
    out = torch.empty(tracks * bufsize, dtype=torch.float32, device=pool.device)
    check(lib.gab_rndmem(_dev(pool), _dev(playheads, torch.int32), _dev(out), tracks, bufsize,
                         _stream()))
    return out


def modal(params, n_modes, bufsize, out_tracks=32):
    out = torch.zeros(out_tracks * bufsize, dtype=torch.float32, device=params.device)
    check(lib.gab_modal(_dev(params), _dev(out), n_modes, bufsize, out_tracks, _stream()))
    return out


def modal_bank_workspace(n_modes, bufsize, out_tracks=32, device="cuda"):
    nbytes = lib.gab_modal_bank_workspace_bytes(n_modes, out_tracks, bufsize)
    return torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=device)


def modal_bank(params, n_modes, bufsize, out_tracks=32, out=None, workspace=None):
    """The real bank (Metal kernel semantics) on 8-float mode records; returns [out_tracks*bufsize]."""
    if out is None:
        out = torch.empty(out_tracks * bufsize, dtype=torch.float32, device=params.device)
    if workspace is None:
        workspace = modal_bank_workspace(n_modes, bufsize, out_tracks, params.device)
    check(lib.gab_modal_bank(_dev(params), _dev(out), n_modes, bufsize, out_tracks, _dev(workspace), _stream()))
    return out


MODAL_FORMS = tuple((J, fixed) for fixed in (1, 0) for J in (1, 2, 4, 8) if fixed or J < 8)


def modal_launch(n_modes, out_tracks=32):
    """(modes per lane, workgroups, 1 if the track count is the kernel's compile-time 32) of gab_modal_bank's launch
    for this shape: gab_debug_modal_launch."""
    J, grid, fixed = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib.gab_debug_modal_launch(n_modes, out_tracks, C.byref(J), C.byref(grid), C.byref(fixed)))
    return J.value, grid.value, fixed.value


DWG_CELLS = ("naive", "one_line", "multi", "lean", "append_staged")
DWG_MIX = ("scan", "gather_sparse", "appended_sparse")


def dwg_route(n_wg, bufsize, max_len=2000, out_tracks=None, variant=DWG_ACCEL):
    """(cells kernel, mix form) gab_dwg takes for this shape, by name (DWG_CELLS, DWG_MIX): gab_debug_dwg_route."""
    cells, mix = C.c_int(0), C.c_int(0)
    check(lib.gab_debug_dwg_route(n_wg, bufsize, max_len, n_wg if out_tracks is None else out_tracks, variant,
                                  C.byref(cells), C.byref(mix)))
    return DWG_CELLS[cells.value], DWG_MIX[mix.value]


def dwg(wg_bytes, fwd, bwd, x, bufsize, max_len=2000, out_tracks=None, variant=DWG_ACCEL):
    """wg_bytes: uint8 device tensor holding n_wg WaveguideState records (32 B each)."""
    n_wg = wg_bytes.numel() // C.sizeof(WaveguideState)
    out = torch.empty(bufsize, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.gab_dwg_workspace_bytes(n_wg, bufsize), dtype=torch.uint8, device=x.device)
    ot = n_wg if out_tracks is None else out_tracks
    check(lib.gab_dwg(_dev(wg_bytes, torch.uint8), _dev(fwd), _dev(bwd), _dev(x), _dev(out),
                      _dev(ws, torch.uint8), n_wg, bufsize, max_len, ot, variant, _stream()))
    return out


def fft_r2c_1024(x, tracks):
    """x: tracks*1024 real -> (tracks, 513, 2) interleaved complex."""
    out = torch.empty(tracks * 513 * 2, dtype=torch.float32, device=x.device)
    check(lib.gab_fft_r2c_1024(_dev(x), _dev(out), tracks, _stream()))
    return out.view(tracks, 513, 2)


class ConvPlan(_Handle):
    """Conv1DAccelBenchmark's device side: spectra bank + history + process()."""

    _destroy = "gab_conv_destroy"
    _SCHEMES = {"classic": 0, "split": 1, "fdl": 2}

    def __init__(self, tracks, bufsize, ir_len, scheme=None):
        """scheme: None (the library's default for this shape), "classic" or "split"
        (gab_conv_set_scheme), or "fdl": long impulse responses through a frequency-domain delay line
        (gab_conv_create_scheme; a plan of that kind from its creation on)."""
        self.tracks, self.bufsize, self.ir_len = tracks, bufsize, ir_len
        self._h = C.c_void_p()
        if scheme == "fdl":
            check(lib.gab_conv_create_scheme(C.byref(self._h), tracks, bufsize, ir_len, self._SCHEMES[scheme]))
            return
        check(lib.gab_conv_create(C.byref(self._h), tracks, bufsize, ir_len))
        if scheme is not None:
            self.set_scheme(scheme)

    def set_scheme(self, scheme):
        check(lib.gab_conv_set_scheme(self._h, self._SCHEMES[scheme]))

    @property
    def scheme(self):
        v = C.c_int(0)
        check(lib.gab_conv_get_scheme(self._h, C.byref(v)))
        return {1: "split", 2: "fdl"}.get(v.value, "classic")

    def set_ir(self, ir):
        assert ir.numel() == self.tracks * self.ir_len
        check(lib.gab_conv_set_ir(self._h, _dev(ir), _stream()))

    def reset(self):
        check(lib.gab_conv_reset(self._h, _stream()))

    def process(self, x, out=None, mode=CONV_STREAMING):
        assert x.numel() == self.tracks * self.bufsize
        if out is None:
            out = torch.empty(self.tracks * self.bufsize, dtype=torch.float32,
                              device=x.device if x.is_cuda else "cuda")
        # x / out may also be pinned host tensors: the kernel then streams the buffer over PCIe
        # itself (zero-copy), without separate copy commands — under its own kernel name
        if mode == CONV_STREAMING and not x.is_cuda and not out.is_cuda:
            mode = CONV_STREAMING_HOST_IO
        check(lib.gab_conv_process(self._h, _acc(x), _acc(out), mode, _stream()))
        return out

    def round_trip(self, h_in, h_out, stream=None):
        """One buffer, pinned host tensor in -> pinned host tensor out; returns when h_out is complete
        (gab_conv_round_trip)."""
        assert h_in.numel() == self.tracks * self.bufsize == h_out.numel()
        if h_in.is_cuda or h_out.is_cuda or not h_out.is_pinned():
            raise TypeError("round_trip takes host tensors; the output must be pinned")
        if h_in.dtype != torch.float32 or h_out.dtype != torch.float32 or not h_in.is_contiguous() or not h_out.is_contiguous():
            raise TypeError("round_trip takes contiguous float32 tensors")
        st = _stream(stream)
        check(lib.gab_conv_round_trip(self._h, C.c_void_p(h_in.data_ptr()), C.c_void_p(h_out.data_ptr()), st))
        return h_out

    def round_trip_check(self):
        """The verdict of the check launch behind the last round trip (gab_conv_round_trip_check): raises if a word the
        kernel consumed early is not what the completed upload left."""
        check(lib.gab_conv_round_trip_check(self._h))

    def round_trip_set_check(self, mode):
        """0 ignore the verdict, 1 (default) read it at the next call / round_trip_check(), 2 read it in the call."""
        check(lib.gab_conv_round_trip_set_check(self._h, int(mode)))

    def round_trip_keep_warm(self, on=True):
        """Every later round trip of this plan ends with a keep-warm kick (gab_conv_round_trip_keep_warm)."""
        check(lib.gab_conv_round_trip_keep_warm(self._h, 1 if on else 0))

    def round_trip_keep_warm_placement(self):
        """KeepWarm.placement() of the plan's own keep-warm launch ([] if it has none)."""
        return _placement(lib.gab_conv_round_trip_keep_warm_placement, self._h)

    def newest_block(self):
        """The block the plan consumed last ([tracks*512], the input's layout), from its history ring
        (gab_conv_newest_block): what a round trip's upload hand-off is checked against."""
        out = torch.empty(self.tracks * self.bufsize, dtype=torch.float32, device="cuda")
        check(lib.gab_conv_newest_block(self._h, _dev(out), _stream()))
        return out

    def prepare_round_trip(self, h_in, h_out, stream=None):
        st = _stream(stream)
        return (self._h, C.c_void_p(h_in.data_ptr()), C.c_void_p(h_out.data_ptr()), st)

    launch_round_trip = _launcher("gab_conv_round_trip")

    # ---- the doorbell-fed resident engine (gab_conv_engine_*) ----
    def engine_rings(self, ring_buffers):
        """The engine's rings without starting it (to fill resident input before the launch takes the device)."""
        a, b = C.c_void_p(), C.c_void_p()
        check(lib.gab_conv_engine_rings(self._h, ring_buffers, C.byref(a), C.byref(b)))
        n = self.tracks * self.bufsize
        return _view(a.value, ring_buffers, n), _view(b.value, ring_buffers, n)

    def engine_start(self, ring_buffers, stream=None):
        """Launches the resident engine; returns (in_ring, out_ring) as device tensors [ring][T*B] / [ring][B*T]
        viewing the plan's rings."""
        a, b = C.c_void_p(), C.c_void_p()
        st = _stream(stream)
        check(lib.gab_conv_engine_start(self._h, ring_buffers, C.byref(a), C.byref(b), st))
        n = self.tracks * self.bufsize
        return _view(a.value, ring_buffers, n), _view(b.value, ring_buffers, n)

    def engine_publish(self, n_more=1):
        check(lib.gab_conv_engine_publish(self._h, n_more))

    def engine_submit(self, n_more=1, flush=True):
        """Publish n_more buffers; flush=True also rings the flush rung: finish what is published without
        waiting for more (the real-time form, one buffer in flight)."""
        check(lib.gab_conv_engine_submit(self._h, n_more, 1 if flush else 0))

    def engine_wait(self, count, timeout=10.0):
        """Spins until `count` buffers are reported complete (gab_conv_engine_wait)."""
        check(lib.gab_conv_engine_wait(self._h, count, float(timeout)))

    def engine_running(self):
        """True while the resident launch is still on the device (gab_conv_engine_running)."""
        v = C.c_int(0)
        check(lib.gab_conv_engine_running(self._h, C.byref(v)))
        return bool(v.value)

    def engine_completed(self):
        v = C.c_int(0)
        check(lib.gab_conv_engine_completed(self._h, C.byref(v)))
        return v.value

    def engine_feed(self, n_buffers, ahead=4):
        check(lib.gab_conv_engine_feed(self._h, n_buffers, ahead))

    def engine_feed_one_in_flight(self, n_buffers, latencies=None):
        """n_buffers times { doorbell with the flush rung; wait for that buffer } on resident rings; latencies: a
        float32 numpy array of n_buffers (host clock, us) or None."""
        ptr = None
        if latencies is not None:
            assert latencies.dtype.name == "float32" and latencies.size >= n_buffers and latencies.flags["C_CONTIGUOUS"]
            ptr = latencies.ctypes.data_as(C.c_void_p)
        check(lib.gab_conv_engine_feed_one_in_flight(self._h, n_buffers, ptr))

    def engine_stop(self):
        check(lib.gab_conv_engine_stop(self._h))

    def engine_round_trip(self, h_in, h_out):
        """Pinned host -> ring slot -> engine (flush rung, ONE buffer in flight) -> ring slot -> pinned host
        (gab_conv_engine_round_trip): the reference's iteration through the resident engine."""
        assert h_in.is_pinned() and h_out.is_pinned() and h_in.numel() == h_out.numel() == self.tracks * self.bufsize
        check(lib.gab_conv_engine_round_trip(self._h, C.c_void_p(h_in.data_ptr()), C.c_void_p(h_out.data_ptr())))

    def engine_set_idle_limit(self, seconds):
        """How long a stalled engine waits for the doorbell before it ends by itself (taken at the next start)."""
        check(lib.gab_conv_engine_set_idle_limit(self._h, float(seconds)))

    def process_batch(self, x, n_buffers, out=None):
        """n_buffers consecutive buffers ([n][T*B] in, [n][B*T] out) in one launch."""
        assert x.numel() == n_buffers * self.tracks * self.bufsize
        if out is None:
            out = torch.empty(n_buffers * self.tracks * self.bufsize, dtype=torch.float32, device=x.device)
        check(lib.gab_conv_process_batch(self._h, _dev(x), _dev(out), n_buffers, _stream()))
        return out

    def prepare_batch(self, x, n_buffers, out, stream=None):
        """The ctypes arguments of process_batch(), built once for a loop over the same resident batch."""
        assert x.numel() == n_buffers * self.tracks * self.bufsize == out.numel()
        st = _stream(stream)
        return (self._h, _dev(x), _dev(out), n_buffers, st)

    launch_batch = _launcher("gab_conv_process_batch")

    def prepare(self, x, out, mode=CONV_STREAMING, stream=None):
        """The ctypes arguments of process(), built once for a loop that cycles through a fixed set
        of buffers; `launch(args)` then costs ~4 us of host time instead of ~7.5."""
        st = _stream(stream)
        return (self._h, _dev(x), _dev(out), mode, st)

    launch = _launcher("gab_conv_process")

    def state_bytes(self):
        a, b = C.c_size_t(0), C.c_size_t(0)
        check(lib.gab_conv_state_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


class EqPlan(_TrackPlan, _Prepared):
    """gab_eq_plan: `sections` biquads in series on each of `tracks` channels, every (track, section) with its own
    coefficients, state carried from buffer to buffer.  A new plan is the identity filter."""

    _destroy = "gab_eq_destroy"

    def __init__(self, tracks, bufsize, sections):
        self.sections = sections
        self._create(tracks, bufsize, sections)

    def set_coeffs(self, coeffs, first_track=None, n_tracks=None):
        """coeffs: device tensor [tracks][sections][5] = {b0,b1,b2,a1,a2} (a0 = 1), or [n_tracks][sections][5]
        for tracks [first_track, first_track + n_tracks)."""
        assert coeffs.numel() == (self.tracks if first_track is None else n_tracks) * self.sections * 5
        self._set("coeffs", _dev(coeffs), first_track, n_tracks)

    def set_sos(self, sos, tracks=None):
        """sos: scipy's second-order sections, [sections][6] = {b0,b1,b2,a0,a1,a2} for every track or
        [tracks][sections][6]; divided by a0.  tracks = (first_track, n_tracks): only those channels
        ([sections][6] for each of them, or [n_tracks][sections][6])."""
        import numpy as np
        sos = np.asarray(sos, np.float64)
        first, n = (0, self.tracks) if tracks is None else (int(tracks[0]), int(tracks[1]))
        if sos.ndim == 2:
            sos = np.broadcast_to(sos, (n,) + sos.shape)
        if sos.shape != (n, self.sections, 6):
            raise ValueError("sos must be [sections][6] or [tracks][sections][6]")
        c = (sos[:, :, [0, 1, 2, 4, 5]] / sos[:, :, 3:4]).astype(np.float32)
        d = torch.from_numpy(np.ascontiguousarray(c)).cuda()
        if tracks is None:
            self.set_coeffs(d)
        else:
            self.set_coeffs(d, first, n)

    def process(self, x, out=None, sequential=False):
        """One buffer, track-major [tracks*bufsize]; out may be x (in place).  sequential=True: the ordered form."""
        return self._process("process_sequential" if sequential else "process", x, out, 1, None, sized=False)

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, None, n, sized=False)

    def state(self):
        """A copy of the carried state, [tracks][sections][2] = (z1, z2)."""
        p, n = C.c_void_p(), C.c_size_t(0)
        check(lib.gab_eq_state(self._h, C.byref(p), C.byref(n)))
        return _view(p.value, n.value // 2, 2).clone().view(self.tracks, self.sections, 2)

    @property
    def form(self):
        """(samples per lane, segments per buffer) of the scan kernel; (0, 0): the sequential kernel only."""
        m, h = C.c_int(0), C.c_int(0)
        check(lib.gab_eq_form(self._h, C.byref(m), C.byref(h)))
        return m.value, h.value

    launch = _launcher("gab_eq_process")


class MixPlan(_TrackPlan):
    """gab_mix_plan: `tracks` channels summed into `buses` buses with a linear gain per (track, bus), in a fixed
    summation order (`form`).  A new plan is silence; new gains are ramped in over the next buffer unless ramp=False."""

    _destroy = "gab_mix_destroy"
    _LAYOUTS = {"track": 0, "sample": 1}

    def __init__(self, tracks, bufsize, buses):
        self.buses = buses
        self._create(tracks, bufsize, buses)

    def set_gains(self, g, ramp=True, first_track=None, n_tracks=None):
        """g: device tensor [tracks][buses], or [n_tracks][buses] for tracks [first_track, first_track + n_tracks)
        (n_tracks=None: as many rows as g holds).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        if first_track is None:
            if n_tracks is not None:
                raise ValueError("n_tracks needs first_track")
            n_tracks = self.tracks
        elif n_tracks is None:                      # the rows g holds
            n_tracks, rest = divmod(g.numel(), self.buses)
            if rest or n_tracks == 0:
                raise ValueError("g must hold whole rows of %d buses" % self.buses)
        assert g.numel() == n_tracks * self.buses
        self._set("gains", _dev(g), first_track, n_tracks, 1 if ramp else 0)

    @staticmethod
    def stereo_gains(gain_db, pan):
        """[tracks][2] float32 for a two-bus plan: constant-power law gL = g cos((pan + 1) pi / 4),
        gR = g sin((pan + 1) pi / 4), g = 10^(gain_db / 20), pan in [-1, 1]; float64, rounded once."""
        import numpy as np
        db, pan = np.broadcast_arrays(np.asarray(gain_db, np.float64), np.asarray(pan, np.float64))
        if pan.size and (pan.min() < -1.0 or pan.max() > 1.0):
            raise ValueError("pan must be in [-1, 1]")
        g = 10.0 ** (db / 20.0)
        th = (pan + 1.0) * (np.pi / 4.0)
        return np.stack([g * np.cos(th), g * np.sin(th)], axis=-1).astype(np.float32)

    def set_stereo(self, gain_db, pan, ramp=True):
        """Per-track level (dB) and pan for a two-bus plan (bus 0 left, bus 1 right); scalars apply to every track."""
        import numpy as np
        if self.buses != 2:
            raise ValueError("set_stereo needs a plan of two buses")
        g = self.stereo_gains(gain_db, pan)
        g = np.array(np.broadcast_to(g, (self.tracks, 2)), np.float32, order="C")
        self.set_gains(torch.from_numpy(g).cuda(), ramp=ramp)

    def reset(self):
        """current := target: a pending ramp is dropped."""
        super().reset()

    def process(self, x, out=None, layout="track"):
        """One buffer: x [tracks*bufsize] track-major ("track") or sample-major ("sample", ConvPlan's output);
        returns [buses*bufsize], bus-major.  out must not overlap x."""
        return self._process("process", x, out, 1, (self.buses * self.bufsize,), self._LAYOUTS[layout])

    def process_batch(self, xs, out=None, layout="track"):
        """Consecutive buffers [n][tracks*bufsize] -> [n][buses*bufsize] in one launch."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, (n * self.buses * self.bufsize,), n, self._LAYOUTS[layout])

    def gains(self):
        """Copies of (current, target), each [tracks][buses]."""
        return self._tables("gains", self.buses)

    @property
    def form(self):
        """(leaf_tracks, group_leaves) of the summation tree; a function of (bufsize, buses) alone."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib.gab_mix_form(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def prepare(self, x, out, layout="track", stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers; `launch(args)`."""
        st = _stream(stream)
        return (self._h, _dev(x), _dev(out), self._LAYOUTS[layout], st)

    launch = _launcher("gab_mix_process")


class DelayPlan(_TrackPlan, _Prepared):
    """gab_delay_plan: a delay line per track, read at a fractional position (interp "linear" or "lagrange3"), with a
    feedback path.  Parameters per track {delay (samples), feedback, wet, dry}; a new plan is pass-through; new
    parameters are ramped in over the next buffer unless ramp=False."""

    _destroy = "gab_delay_destroy"
    _INTERP = {"linear": 0, "lagrange3": 1}

    def __init__(self, tracks, bufsize, max_delay, interp="linear"):
        if interp not in self._INTERP:
            raise ValueError("interp must be 'linear' or 'lagrange3'")
        self.max_delay, self.interp = max_delay, interp
        self.min_delay = 2 if interp == "lagrange3" else 1
        self._create(tracks, bufsize, max_delay, self._INTERP[interp])

    def set_params(self, params, ramp=True, first_track=0):
        """params: device tensor [n][4] = {delay, feedback, wet, dry} for tracks [first_track, first_track + n).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        n = self._rows(params, 4, first_track, "params")
        whole = first_track == 0 and n == self.tracks           # (first_track has a number by default: any n goes)
        self._set("params", _dev(params), None if whole else first_track, n, 1 if ramp else 0)

    def reset(self):
        """Zero lines, current := target, a pending ramp dropped."""
        super().reset()

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize]; out may be x itself."""
        return self._process("process", x, out, 1, None)

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, None, n)

    def params(self):
        """Copies of (current, target), each [tracks][4]."""
        return self._tables("params", 4)

    def line(self):
        """Copies of (ring [tracks][capacity] float32, write positions [tracks] int64)."""
        r, p, cap = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        check(lib.gab_delay_line(self._h, C.byref(r), C.byref(cap), C.byref(p)))
        return _view(r.value, self.tracks, cap.value).clone(), _positions(p.value, self.tracks)

    launch = _launcher("gab_delay_process")


def dynamics_params(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db=0.0, range_db=None, fs=48000.0):
    """A row (all arguments scalars) or a table [n][8] float32 of DynamicsPlan parameters {thr, slope, knee, kq, att,
    rel, makeup, range} from the knobs of a compressor; float64, rounded once.  Levels go from dB to log2 units
    (6.0206 dB each); knee_db is the knee's whole width; ratio = inf is a limiter; a time of 0 ms is a coefficient
    of 0, else exp(-1 / (ms fs / 1000)); range_db=None leaves the reduction unbounded (-256 units)."""
    import numpy as np
    unit = 20.0 * np.log10(2.0)
    args = [np.asarray(a, np.float64) for a in (threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db,
                                                -256.0 * unit if range_db is None else range_db)]
    scalar = all(a.ndim == 0 for a in args)
    thr_db, ratio, knee_db, att_ms, rel_ms, makeup_db, range_db = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    if (ratio < 1.0).any() or (knee_db < 0.0).any() or (att_ms < 0.0).any() or (rel_ms < 0.0).any() or (range_db > 0.0).any():
        raise ValueError("needs ratio >= 1, knee_db >= 0, attack_ms >= 0, release_ms >= 0, range_db <= 0")
    knee = 0.5 * knee_db / unit
    with np.errstate(divide="ignore"):
        kq = np.where(knee > 0.0, 1.0 / (4.0 * np.where(knee > 0.0, knee, 1.0)), 0.0)
        att = np.where(att_ms > 0.0, np.exp(-1.0 / np.where(att_ms > 0.0, att_ms * fs / 1000.0, 1.0)), 0.0)
        rel = np.where(rel_ms > 0.0, np.exp(-1.0 / np.where(rel_ms > 0.0, rel_ms * fs / 1000.0, 1.0)), 0.0)
        slope = 1.0 / ratio - 1.0                                    # inf: -1
    cap = 1.0 - 2.0 ** -20                                           # the plan's cap on a coefficient: 22 s at 48 kHz
    table = np.stack([thr_db / unit, slope, knee, kq, np.minimum(att, cap), np.minimum(rel, cap),
                      10.0 ** (makeup_db / 20.0), np.maximum(range_db / unit, -256.0)], axis=-1).astype(np.float32)
    return table[0] if scalar else table


class DynamicsPlan(_KeyedPlan):
    """gab_dyn_plan: a compressor / limiter per track with a carried smoothed gain.  Parameters per track {thr, slope,
    knee, kq, att, rel, makeup, range} (dynamics_params makes them from dB, ratio and ms); tracks [g link, (g + 1) link)
    share one detector.  A new plan is pass-through; new parameters are ramped in over the next buffer unless
    ramp=False."""

    _destroy = "gab_dyn_destroy"
    FIELDS = ("thr", "slope", "knee", "kq", "att", "rel", "makeup", "range")

    def reset(self):
        """The smoothed gain zero, current := target, a pending ramp dropped."""
        super().reset()

    def process(self, x, key=None, out=None, gr=None):
        """One buffer, track-major [tracks*bufsize]; out may be x itself.  key: the side chain the detector reads instead
        of x (may not overlap out).  gr: a tensor [tracks] that receives the buffer's smallest smoothed gain."""
        return self._run("process", x, key, out, gr, None)

    def process_batch(self, xs, key=None, out=None, gr=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch; key the same shape, gr [n][tracks]."""
        return self._run("process_batch", xs, key, out, gr, _n_buffers(self, xs))

    def state(self):
        """A copy of the smoothed gain, [tracks], log2 units."""
        p, n = C.c_void_p(), C.c_size_t(0)
        check(lib.gab_dyn_state(self._h, C.byref(p), C.byref(n)))
        return _view(p.value, self.tracks, 1).clone().view(self.tracks)

    def prepare(self, x, out, key=None, gr=None, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  All state that changes is on the device; which kernel form runs (steady, or the ramp form when
        a ramp is pending) is the host's choice at the call and what a capture replays: gab_c_api.h, "Captured calls"."""
        return (self._h, _dev(x), None if key is None else _dev(key), _dev(out), None if gr is None else _dev(gr),
                _stream(stream))

    launch = _launcher("gab_dyn_process")


def gate_params(open_db, close_db=None, attack_ms=1.0, release_ms=100.0, hold_ms=10.0, range_db=None, duck_db=None,
                fs=48000.0):
    """A row (all arguments scalars) or a table [n][7] float32 of GatePlan parameters {open, close, att, rel, g_open,
    g_closed, hold} from the knobs of a gate; float64, rounded once.  Thresholds go from dB to linear levels; close_db
    defaults to 3 dB under open_db; a time of 0 ms is a coefficient of 0, else exp(-1 / (ms fs / 1000)), held to the
    plan's 1 - 2^-20; hold_ms becomes a whole number of samples.  A noise gate: g_open = 1 and g_closed from range_db
    (<= 0; None: 0, the gate shuts).  duck_db (<= 0) given makes the ducker's row instead: g_open = that depth,
    g_closed = 1, to be run with the voice as the key."""
    import numpy as np
    if duck_db is not None and range_db is not None:
        raise ValueError("range_db belongs to a gate, duck_db to a ducker: give one")
    args = [np.asarray(a, np.float64) for a in (open_db, open_db if close_db is None else close_db, attack_ms, release_ms,
                                                hold_ms, 0.0 if range_db is None else range_db,
                                                0.0 if duck_db is None else duck_db)]
    scalar = all(a.ndim == 0 for a in args)
    open_db, close_db_, att_ms, rel_ms, hold_ms, range_db_, duck_db_ = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    if close_db is None:
        close_db_ = open_db - 3.0
    if ((close_db_ > open_db).any() or (att_ms < 0.0).any() or (rel_ms < 0.0).any() or (hold_ms < 0.0).any()
            or (range_db_ > 0.0).any() or (duck_db_ > 0.0).any() or fs <= 0.0):
        raise ValueError("needs close_db <= open_db, attack_ms, release_ms, hold_ms >= 0, range_db <= 0, duck_db <= 0, fs > 0")
    att = np.where(att_ms > 0.0, np.exp(-1.0 / np.where(att_ms > 0.0, att_ms * fs / 1000.0, 1.0)), 0.0)
    rel = np.where(rel_ms > 0.0, np.exp(-1.0 / np.where(rel_ms > 0.0, rel_ms * fs / 1000.0, 1.0)), 0.0)
    cap = 1.0 - 2.0 ** -20                                           # the plan's cap on a coefficient: 22 s at 48 kHz
    one = np.ones_like(open_db)
    if duck_db is None:
        g_open, g_closed = one, (0.0 * one if range_db is None else 10.0 ** (range_db_ / 20.0))
    else:
        g_open, g_closed = 10.0 ** (duck_db_ / 20.0), one
    table = np.stack([np.minimum(10.0 ** (open_db / 20.0), 2.0 ** 64), np.minimum(10.0 ** (close_db_ / 20.0), 2.0 ** 64),
                      np.minimum(att, cap), np.minimum(rel, cap), g_open, g_closed,
                      np.minimum(np.rint(hold_ms * fs / 1000.0), 2.0 ** 24)], axis=-1).astype(np.float32)
    return table[0] if scalar else table


class GatePlan(_KeyedPlan):
    """gab_gate_plan: a noise gate or ducker per track: a two-state machine with hysteresis (open above `open`, the hold
    runs down below `close`) and a hold counter, and a linear gain that glides to g_open or g_closed.  Parameters per
    track {open, close, att, rel, g_open, g_closed, hold} (gate_params makes them from dB and ms); tracks [g link,
    (g + 1) link) share one detector.  A new plan is pass-through; new parameters are ramped in over the next buffer
    unless ramp=False (the hold is never ramped)."""

    _destroy = "gab_gate_destroy"
    FIELDS = ("open", "close", "att", "rel", "g_open", "g_closed", "hold")
    _extra = torch.int32

    def reset(self):
        """Every gate shut at target's g_closed, current := target, a pending ramp dropped."""
        super().reset()

    def process(self, x, key=None, out=None, act=None):
        """One buffer, track-major [tracks*bufsize]; out may be x itself.  key: the side chain the detector reads instead
        of x (may not overlap out).  act: an int32 tensor [tracks] that receives the buffer's count of open samples."""
        return self._run("process", x, key, out, act, None)

    def process_batch(self, xs, key=None, out=None, act=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch; key the same shape, act [n][tracks] int32."""
        return self._run("process_batch", xs, key, out, act, _n_buffers(self, xs))

    def state(self):
        """Copies of (the gain [tracks] float32, the count [tracks] int32: -1 while closed)."""
        g, c, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        check(lib.gab_gate_state(self._h, C.byref(g), C.byref(c), C.byref(n)))
        return (_view(g.value, self.tracks, 1).clone().view(self.tracks),
                _view(c.value, self.tracks, 1).clone().view(torch.int32).view(self.tracks))

    def prepare(self, x, out, key=None, act=None, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  All state that changes is on the device; which kernel form runs (steady, or the ramp form when
        a ramp is pending) is the host's choice at the call and what a capture replays, so capture only with no ramp
        pending: gab_c_api.h, "Captured calls"."""
        return (self._h, _dev(x), None if key is None else _dev(key), _dev(out),
                None if act is None else _dev(act, torch.int32), _stream(stream))

    launch = _launcher("gab_gate_process")


XOVER_K32 = 1.41421353816986083984375      # (float)sqrt(2.0), GAB_XOVER_K32: the damping of a crossover section


def crossover_rows(freqs_hz, fs=48000.0):
    """CrossoverPlan's table from split frequencies: a scalar (one split), a list of S ascending frequencies (every
    track the same) or [T][S]; each within (0, fs / 2).  Returns float32 [T or 1][S][3] = {a1, a2, a3} per split:
    g = tan(pi f / fs), a1 = 1 / (1 + g (g + K32)), a2 = g a1, a3 = g a2, in float64, rounded once."""
    import numpy as np
    f = np.asarray(freqs_hz, np.float64)
    if f.ndim > 2 or f.size == 0:
        raise ValueError("freqs_hz must be a scalar, [S] or [T][S]")
    f = f.reshape((1, -1)) if f.ndim < 2 else f
    if not fs > 0.0 or not (np.isfinite(f).all() and (f > 0.0).all() and (f < fs / 2.0).all()):
        raise ValueError("every split frequency must be within (0, fs / 2)")
    if not (np.diff(f, axis=1) > 0.0).all():
        raise ValueError("the split frequencies of a track must ascend")
    g = np.tan(np.pi * f / fs)
    a1 = 1.0 / (1.0 + g * (g + XOVER_K32))
    a2 = g * a1
    return np.stack([a1, a2, g * a2], axis=-1).astype(np.float32)


class CrossoverPlan(_TrackPlan, _Prepared):
    """gab_xover_plan: every track split into `bands` = 2..4 bands by Linkwitz-Riley (fourth-order) crossovers, band 0
    the lowest; the bands sum to the input through an all-pass.  Rows {a1, a2, a3} per (track, split) come from
    crossover_rows.  A new plan has no rows: set_splits comes before process.  Splits are not ramped."""

    _destroy = "gab_xover_destroy"

    def __init__(self, tracks, bufsize, bands):
        self.bands = bands
        self._create(tracks, bufsize, bands)
        self.splits_per_track = bands - 1

    @staticmethod
    def sections(bands):
        """The sections of a track: 3, 7, 12 for 2, 3, 4 bands (0: not a band count of the plan)."""
        return lib.gab_xover_sections(bands)

    def set_splits(self, rows, first_track=None, n_tracks=None):
        """rows: device tensor [tracks][bands - 1][3], or [n_tracks][bands - 1][3] for tracks [first_track, first_track +
        n_tracks) (n_tracks=None: as many as rows holds).  Acts from the next buffer; the state is kept."""
        if first_track is None and n_tracks is not None:
            raise ValueError("n_tracks needs first_track")
        n = self._rows(rows, 3 * self.splits_per_track, first_track, "rows")
        if n_tracks is not None and n != n_tracks:
            raise ValueError("rows must hold n_tracks tracks")
        self._set("splits", _dev(rows), first_track, n)

    def reset(self):
        """Every state to zero; the rows are kept."""
        super().reset()

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize] -> [bands][tracks*bufsize], band-major; out may not overlap x."""
        return self._process("process", x, out, 1, (self.bands * self.tracks * self.bufsize,))

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] -> [n][bands][tracks*bufsize] in one launch."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, (n * self.bands * self.tracks * self.bufsize,), n)

    def splits(self):
        """A copy of the table, [tracks][bands - 1][3]."""
        p, n = C.c_void_p(), C.c_size_t(0)
        check(lib.gab_xover_splits(self._h, C.byref(p), C.byref(n)))
        return _view(p.value, n.value // 3, 3).clone().view(self.tracks, self.splits_per_track, 3)

    def state(self):
        """A copy of the carried state, [tracks][sections][2] = (ic1, ic2), the sections in the header's order."""
        p, n = C.c_void_p(), C.c_size_t(0)
        check(lib.gab_xover_state(self._h, C.byref(p), C.byref(n)))
        return _view(p.value, n.value // 2, 2).clone().view(self.tracks, -1, 2)

    launch = _launcher("gab_xover_process")


def limiter_params(ceiling_db=-1.0, release_ms=100.0, drive_db=0.0, fs=48000.0):
    """A row (all arguments scalars) or a table [n][3] float32 of LimiterPlan parameters {drive, ceil, rel} from the
    knobs of a limiter; float64, rounded once.  Levels go from dB to linear; rel = 1 - exp(-1 / (release_s fs)), and
    release_ms = 0 gives rel = 1 (the gain is back W samples behind a peak)."""
    import numpy as np
    args = [np.asarray(a, np.float64) for a in (ceiling_db, release_ms, drive_db)]
    scalar = all(a.ndim == 0 for a in args)
    ceil_db, rel_ms, drive_db = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    if (rel_ms < 0.0).any() or fs <= 0.0:
        raise ValueError("needs release_ms >= 0 and fs > 0")
    rel = np.where(rel_ms > 0.0, 1.0 - np.exp(-1.0 / np.where(rel_ms > 0.0, rel_ms * fs / 1000.0, 1.0)), 1.0)
    table = np.stack([10.0 ** (drive_db / 20.0), 10.0 ** (ceil_db / 20.0), rel], axis=-1).astype(np.float32)
    return table[0] if scalar else table


class LimiterPlan(_TrackPlan):
    """gab_lim_plan: a brickwall look-ahead limiter per track: |y| <= ceil on every sample, bit for bit the contract of
    gab_c_api.h.  `lookahead` is the window W, a power of two in 4..256; the plan delays by `.latency` = W - 1 samples.
    Parameters per track {drive, ceil, rel} (limiter_params makes them from dB and ms); tracks [g link, (g + 1) link)
    share one detector.  A new plan is a pure delay; new parameters are ramped in over the next buffer unless
    ramp=False."""

    _destroy = "gab_lim_destroy"
    FIELDS = ("drive", "ceil", "rel")

    def __init__(self, tracks, bufsize, lookahead=64, link=1):
        k = int(lookahead).bit_length() - 1
        if lookahead != 1 << max(k, 0):
            raise ValueError("lookahead must be a power of two in 4..256")
        self.lookahead, self.link = lookahead, link
        self._create(tracks, bufsize, k, link)
        n = C.c_int(0)
        check(lib.gab_lim_latency(self._h, C.byref(n)))
        self.latency = n.value

    def set_params(self, table, ramp=True, first_track=None):
        """table: device tensor [tracks][3], or [n][3] for tracks [first_track, first_track + n).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        n = self._rows(table, len(self.FIELDS), first_track)
        self._set("params", _dev(table), first_track, n, 1 if ramp else 0)

    def reset(self):
        """The histories as in a new plan (xd = 0, t = 1, e = 1), current := target, a pending ramp dropped."""
        super().reset()

    def _gr(self, gr, n):
        assert gr is None or gr.numel() == n * self.tracks
        return None if gr is None else _dev(gr)

    def process(self, x, out=None, gr=None):
        """One buffer, track-major [tracks*bufsize]; out may be x itself.  gr: a tensor [tracks] that receives the
        buffer's smallest gain."""
        return self._process("process", x, out, 1, None, self._gr(gr, 1))

    def process_batch(self, xs, out=None, gr=None):
        """Consecutive buffers [n][tracks*bufsize]; gr [n][tracks]."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, None, self._gr(gr, n), n)

    def params(self):
        """Copies of (current, target), each [tracks][3]."""
        return self._tables("params", len(self.FIELDS))

    def state(self):
        """Copies of the three histories (xd, t, e), each [tracks][W - 1], oldest first."""
        x, t, e, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        check(lib.gab_lim_state(self._h, C.byref(x), C.byref(t), C.byref(e), C.byref(n)))
        return tuple(_view(p.value, self.tracks, n.value).clone() for p in (x, t, e))

    def prepare(self, x, out, gr=None, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  All state that changes is on the device; which kernel form runs (steady, or the ramp form when
        a ramp is pending) is the host's choice at the call and what a capture replays, so capture only with no ramp
        pending: gab_c_api.h, "Captured calls"."""
        return (self._h, _dev(x), _dev(out), None if gr is None else _dev(gr), _stream(stream))

    launch = _launcher("gab_lim_process")


def saturator_params(drive_db=0.0, bias=0.0, level_db=0.0, compensate=False):
    """A row (all arguments scalars) or a table [n][3] float32 of SaturatorPlan parameters {drive, bias, level} from the
    knobs of a saturator; float64, rounded once.  Levels go from dB to linear; compensate=True divides level by drive,
    so that a signal below the curve's knee keeps its level whatever the drive."""
    import numpy as np
    args = [np.asarray(a, np.float64) for a in (drive_db, bias, level_db)]
    scalar = all(a.ndim == 0 for a in args)
    drive_db, bias, level_db = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    drive = 10.0 ** (drive_db / 20.0)
    level = 10.0 ** (level_db / 20.0)
    if compensate:
        level = level / drive
    table = np.stack([drive, bias, level], axis=-1).astype(np.float32)
    return table[0] if scalar else table


class SaturatorPlan(_TrackPlan):
    """gab_sat_plan: a waveshaper per track at `oversample` (1, 2, 4 or 8) times the stream's rate, so that the harmonics
    it makes do not fold back: up by R, the curve ("hard", "cubic" or "rational"), down by R in one launch, bit for bit
    ResamplePlan(up=R) -> apply -> ResamplePlan(down=R) (gab_c_api.h).  Parameters per track {drive, bias, level}
    (saturator_params makes them from dB); a new plan holds {1, 0, 1}, and new parameters are ramped in over the next
    buffer unless ramp=False.  up_taps / down_taps None: ResamplePlan.default_taps, 32 and 32 R (0 and 0 at R = 1).
    The plan delays by `.latency` = up_taps / 2 + down_taps / (2 R) samples."""

    _destroy = "gab_sat_destroy"
    FIELDS = ("drive", "bias", "level")
    CURVES = ("hard", "cubic", "rational")

    def __init__(self, tracks, bufsize, oversample=4, curve="cubic", up_taps=None, down_taps=None):
        if curve not in self.CURVES:
            raise ValueError("curve must be one of %s" % (self.CURVES,))
        if oversample == 1:
            up_taps, down_taps = up_taps or 0, down_taps or 0
        elif oversample in (2, 4, 8):
            up_taps = ResamplePlan.default_taps(oversample, 1) if up_taps is None else up_taps
            down_taps = ResamplePlan.default_taps(1, oversample) if down_taps is None else down_taps
        else:
            up_taps, down_taps = up_taps or 0, down_taps or 0         # the library refuses it with its text
        self._create(tracks, bufsize, oversample, self.CURVES.index(curve), up_taps, down_taps)
        v = [C.c_int(0) for _ in range(5)]
        check(lib.gab_sat_info(self._h, *[C.byref(c) for c in v]))
        self.oversample, _, self.up_taps, self.down_taps, self.latency = (c.value for c in v)
        self.curve = curve

    def set_params(self, table, ramp=True, first_track=None):
        """table: device tensor [tracks][3], or [n][3] for tracks [first_track, first_track + n).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        n = self._rows(table, len(self.FIELDS), first_track)
        self._set("params", _dev(table), first_track, n, 1 if ramp else 0)

    def set_taps(self, up, down):
        """up: device tensor [oversample][up_taps], down: [down_taps]; in force from the next buffer, the histories are
        kept."""
        assert up.numel() == self.oversample * self.up_taps and down.numel() == self.down_taps
        check(lib.gab_sat_set_taps(self._h, _dev(up), _dev(down), _stream()))

    def reset(self):
        """Both histories zero, current := target, a pending ramp dropped; the taps stay."""
        super().reset()

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize]; out may not overlap x."""
        return self._process("process", x, out, 1, None)

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, None, n)

    def apply(self, u, out=None):
        """The curve alone on oversampled blocks [n][tracks][oversample*bufsize] (what ResamplePlan(up=oversample) gives);
        out may be u itself.  Takes a pending ramp as process_batch would; touches no history."""
        n, rest = divmod(u.numel(), self.tracks * self.bufsize * self.oversample)
        assert rest == 0
        out = torch.empty_like(u) if out is None else out
        assert out.numel() == u.numel()
        check(lib.gab_sat_apply(self._h, _dev(u), _dev(out), n, _stream()))
        return out

    def params(self):
        """Copies of (current, target), each [tracks][3]."""
        return self._tables("params", len(self.FIELDS))

    def _state(self):
        p = [C.c_void_p() for _ in range(4)]
        check(lib.gab_sat_state(self._h, *[C.byref(c) for c in p]))
        return [c.value for c in p]

    def state(self):
        """Copies of (hist_in [tracks][up_taps-1], hist_os [tracks][down_taps-1]), oldest first; (None, None) at
        oversample 1."""
        if self.oversample == 1:
            return None, None
        a, b, _, _ = self._state()
        return _view(a, self.tracks, self.up_taps - 1).clone(), _view(b, self.tracks, self.down_taps - 1).clone()

    def taps(self):
        """Copies of the tables in force, (up [oversample][up_taps], down [down_taps]); (None, None) at oversample 1."""
        if self.oversample == 1:
            return None, None
        _, _, u, d = self._state()
        return _view(u, self.oversample, self.up_taps).clone(), _view(d, 1, self.down_taps).clone().view(-1)

    def prepare(self, x, out, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  Capture only with no ramp pending: gab_c_api.h, "Captured calls"."""
        return (self._h, _dev(x), _dev(out), _stream(stream))

    launch = _launcher("gab_sat_process")


def nlms_params(step=0.5, floor_db=-60.0, taps=64):
    """A row (all arguments scalars) or a table [n][2] float32 of NlmsPlan parameters {mu, eps} from the knobs of an
    echo canceller; float64, rounded once.  mu = step; eps = taps * 10^(floor_db / 10): the window power of a reference
    at floor_db, below which the normalisation stops raising the step."""
    import numpy as np
    args = [np.asarray(a, np.float64) for a in (step, floor_db, taps)]
    scalar = all(a.ndim == 0 for a in args)
    step, floor_db, taps = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    table = np.stack([step, taps * 10.0 ** (floor_db / 10.0)], axis=-1).astype(np.float32)
    return table[0] if scalar else table


class NlmsPlan(_TrackPlan):
    """gab_nlms_plan: a normalised-LMS adaptive filter per track (an echo canceller), bit for bit the contract of
    gab_c_api.h.  Per track it reads a reference `ref` and an input `x`, writes the estimate (ref through the track's
    `taps` taps: 64, 128, 256 or 512) and the error x - estimate, and adapts the taps on every sample.  Parameters per
    track {mu, eps} (nlms_params makes them); a new plan holds zero taps and {0, 1}: the error is x and the estimate +0.
    With mu = 0 and set_taps it is an FIR filter with its own taps per track.  New parameters are ramped in over the
    next buffer unless ramp=False."""

    _destroy = "gab_nlms_destroy"
    FIELDS = ("mu", "eps")

    def __init__(self, tracks, bufsize, taps=64):
        self.taps = taps
        self._create(tracks, bufsize, taps)

    def set_params(self, table, ramp=True, first_track=None):
        """table: device tensor [tracks][2], or [n][2] for tracks [first_track, first_track + n).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        n = self._rows(table, len(self.FIELDS), first_track)
        self._set("params", _dev(table), first_track, n, 1 if ramp else 0)

    def set_taps(self, w, first_track=None):
        """w: device tensor [tracks][taps], or [n][taps] for tracks [first_track, first_track + n); finite values, in
        force at once; the history stays."""
        n = self._rows(w, self.taps, first_track, "taps")
        self._set("taps", _dev(w), first_track, n)

    def reset(self):
        """Taps and history zero, current := target, a pending ramp dropped."""
        super().reset()

    def _run(self, what, x, ref, err, est, n):
        assert x.numel() == (n or 1) * self.tracks * self.bufsize and ref.numel() == x.numel()
        if err is None and est is None:
            err = torch.empty_like(x)
        assert all(o is None or o.numel() == x.numel() for o in (err, est))
        rest = () if n is None else (n,)
        check(self._fn(what)(self._h, _dev(x), _dev(ref), None if err is None else _dev(err),
                             None if est is None else _dev(est), *rest, _stream()))
        return err, est

    def process(self, x, ref, err=None, est=None):
        """One buffer, track-major [tracks*bufsize]: x the input (the microphone), ref the reference (the far end).
        Returns (err, est).  err may be x itself and est may be ref itself.  With neither given a new err is made and
        est is None; with one given the other is not computed."""
        return self._run("process", x, ref, err, est, None)

    def process_batch(self, xs, refs, err=None, est=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch."""
        return self._run("process_batch", xs, refs, err, est, _n_buffers(self, xs))

    def params(self):
        """Copies of (current, target), each [tracks][2]."""
        return self._tables("params", len(self.FIELDS))

    def state(self):
        """Copies of (taps [tracks][taps], history [tracks][taps - 1], the last reference samples, oldest first)."""
        w, h, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib.gab_nlms_state(self._h, C.byref(w), C.byref(h), C.byref(n)))
        return _view(w.value, self.tracks, n.value).clone(), _view(h.value, self.tracks, n.value - 1).clone()

    def prepare(self, x, ref, err=None, est=None, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  Capture only with no ramp pending: gab_c_api.h, "Captured calls"."""
        return (self._h, _dev(x), _dev(ref), None if err is None else _dev(err), None if est is None else _dev(est),
                _stream(stream))

    launch = _launcher("gab_nlms_process")


def fdaf_params(step=0.5, floor_db=-60.0, partitions=1):
    """A row (all arguments scalars) or a table [n][2] float32 of FdafPlan parameters {mu, eps} from the knobs of an
    echo canceller; float64, rounded once.  mu = step; eps = partitions * 1024 * 10^(floor_db / 10): the bin power, in
    the units of the unnormalised 1024-point transform, of a white reference at floor_db, below which the normalisation
    stops raising the step.  One partition diverges at step 1 and is fine at 0.5; four and more take 1."""
    import numpy as np
    args = [np.asarray(a, np.float64) for a in (step, floor_db, partitions)]
    scalar = all(a.ndim == 0 for a in args)
    step, floor_db, partitions = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    table = np.stack([step, partitions * 1024.0 * 10.0 ** (floor_db / 10.0)], axis=-1).astype(np.float32)
    return table[0] if scalar else table


class FdafPlan(_TrackPlan):
    """gab_fdaf_plan: a partitioned frequency-domain NLMS filter per track (the multidelay block filter), the long form
    of NlmsPlan: `partitions` K in 1..32 of 512 taps each, adapted per bin once per block of 512 samples; bufsize a
    multiple of 512.  Per track it reads a reference `ref` and an input `x` and writes the estimate (ref through the
    taps) and the error x - estimate.  Parameters per track {mu, eps} (fdaf_params makes them), in force from the next
    block: there is no ramp.  A new plan holds zero taps and {0, 1}: the error is x and the estimate +0.  With mu = 0 and
    set_taps it is a partitioned FIR filter with its own long taps per track."""

    _destroy = "gab_fdaf_destroy"
    FIELDS = ("mu", "eps")
    BLOCK, BINS = 512, 513

    def __init__(self, tracks, bufsize, partitions=1):
        self.partitions = partitions
        self._create(tracks, bufsize, partitions)

    def set_params(self, table, first_track=None):
        """table: device tensor [tracks][2], or [n][2] for tracks [first_track, first_track + n); at once."""
        n = self._rows(table, len(self.FIELDS), first_track)
        self._set("params", _dev(table), first_track, n)

    def set_taps(self, h, first_track=None):
        """h: device tensor [tracks][512 partitions] of time-domain taps, or [n][...] for tracks [first_track,
        first_track + n); finite values, in force at once; the delay line and the block count stay."""
        n = self._rows(h, self.BLOCK * self.partitions, first_track, "taps")
        self._set("taps", _dev(h), first_track, n)

    def reset(self):
        """Taps, delay line, previous block and block count zero; the parameters stay."""
        super().reset()

    def _run(self, what, x, ref, err, est, n):
        assert x.numel() == (n or 1) * self.tracks * self.bufsize and ref.numel() == x.numel()
        if err is None and est is None:
            err = torch.empty_like(x)
        assert all(o is None or o.numel() == x.numel() for o in (err, est))
        rest = () if n is None else (n,)
        check(self._fn(what)(self._h, _dev(x), _dev(ref), None if err is None else _dev(err),
                             None if est is None else _dev(est), *rest, _stream()))
        return err, est

    def process(self, x, ref, err=None, est=None):
        """One buffer, track-major [tracks*bufsize]: x the input (the microphone), ref the reference (the far end).
        Returns (err, est).  err may be x itself and est may be ref itself.  With neither given a new err is made and
        est is None; with one given the other is not computed."""
        return self._run("process", x, ref, err, est, None)

    def process_batch(self, xs, refs, err=None, est=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch."""
        return self._run("process_batch", xs, refs, err, est, _n_buffers(self, xs))

    def params(self):
        """A copy of the table [tracks][2]."""
        p, n = C.c_void_p(), C.c_size_t(0)
        check(lib.gab_fdaf_params(self._h, C.byref(p), C.byref(n)))
        return _view(p.value, self.tracks, len(self.FIELDS)).clone()

    def state(self):
        """Copies of (W [tracks][K][513] complex64, the partitions' half-spectra; X, the same shape, the delay line with
        block b in slot b mod K; prev [tracks][512], the reference block before; count [tracks] int64, the blocks since
        the reset)."""
        w, x, pv, c, k = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib.gab_fdaf_state(self._h, C.byref(w), C.byref(x), C.byref(pv), C.byref(c), C.byref(k)))
        shape = (self.tracks, k.value, self.BINS)
        spectra = [torch.view_as_complex(_view(p.value, self.tracks, k.value * self.BINS * 2).clone()
                                         .view(*shape, 2)) for p in (w, x)]
        return spectra[0], spectra[1], _view(pv.value, self.tracks, self.BLOCK).clone(), _positions(c.value, self.tracks)

    def taps(self):
        """The taps in time [tracks][512 partitions]: the first 512 samples of each partition's inverse transform, by
        torch.fft on a copy of W."""
        w = self.state()[0]
        return torch.fft.irfft(w, n=2 * self.BLOCK, dim=-1)[..., :self.BLOCK].reshape(self.tracks, -1).contiguous()

    def prepare(self, x, ref, err=None, est=None, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`."""
        return (self._h, _dev(x), _dev(ref), None if err is None else _dev(err), None if est is None else _dev(est),
                _stream(stream))

    launch = _launcher("gab_fdaf_process")


class MatrixConvPlan(_TrackPlan, _Prepared):
    """gab_mconv_plan: `inputs` channels summed into `outputs` channels through a partitioned FIR filter per (output,
    input): `partitions` K in 1..32 of 512 taps each; bufsize a multiple of 512.  A binaural renderer, a true-stereo
    reverb, an array decoder.  x is [inputs*bufsize], the result [outputs*bufsize], bus-major as MixPlan writes.  A new
    plan holds zero taps: silence.  New taps are crossfaded in over the next buffer unless ramp=False."""

    _destroy = "gab_mconv_destroy"
    BLOCK, BINS = 512, 513

    def __init__(self, inputs, outputs, bufsize, partitions=1):
        self.inputs, self.outputs, self.partitions = inputs, outputs, partitions
        self._create(inputs, bufsize, outputs, partitions)

    def set_taps(self, h, ramp=True, first_output=None, first_input=None):
        """h: device tensor [outputs][inputs][512 partitions] of finite time-domain taps.  With first_output and / or
        first_input (the other then starts at 0) h is a 3-d [n_out][n_in][512 partitions] for outputs [first_output,
        first_output + n_out) x inputs [first_input, first_input + n_in).  ramp=True: the next buffer processed is the
        blend from the old taps' output to the new taps'; ramp=False: in force from the next block."""
        L = self.BLOCK * self.partitions
        ramped = 1 if ramp else 0
        if first_output is None and first_input is None:
            if h.numel() != self.outputs * self.inputs * L:
                raise ValueError("taps must hold [outputs][inputs][%d] values (or give first_output / first_input)" % L)
            check(lib.gab_mconv_set_taps(self._h, _dev(h), ramped, _stream()))
            return
        if h.dim() != 3 or h.shape[2] != L or h.shape[0] == 0 or h.shape[1] == 0:
            raise ValueError("the taps of a range must be [n_out][n_in][%d]" % L)
        check(lib.gab_mconv_set_taps_range(self._h, _dev(h), first_output or 0, h.shape[0], first_input or 0, h.shape[1],
                                           ramped, _stream()))

    def reset(self):
        """The ring, the previous block and the block count zero; the taps stay and a pending ramp is dropped."""
        super().reset()

    def process(self, x, out=None):
        """One buffer: x [inputs*bufsize] -> [outputs*bufsize].  out must not overlap x."""
        return self._process("process", x, out, 1, (self.outputs * self.bufsize,))

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][inputs*bufsize] -> [n][outputs*bufsize]; a pending ramp runs through the first."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, (n * self.outputs * self.bufsize,), n)

    def state(self):
        """Copies of (H_current, H_target [outputs][inputs][K][513] complex64, the taps' half-spectra; X [K + 15][inputs]
        [513] complex64, the ring with block b in slot b mod (K + 15); prev [inputs][512], the input block before;
        count, the blocks since the reset)."""
        hc, ht, x, pv, c, s = (C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0))
        check(lib.gab_mconv_state(self._h, C.byref(hc), C.byref(ht), C.byref(x), C.byref(pv), C.byref(c), C.byref(s)))

        def spectra(p, *shape):
            rows = shape[0]
            flat = _view(p.value, rows, torch.Size(shape[1:]).numel() * 2).clone()
            return torch.view_as_complex(flat.view(*shape, 2))
        taps = (self.outputs, self.inputs, self.partitions, self.BINS)
        return (spectra(hc, *taps), spectra(ht, *taps), spectra(x, s.value, self.inputs, self.BINS),
                _view(pv.value, self.inputs, self.BLOCK).clone(), int(_positions(c.value, 1)[0]))

    launch = _launcher("gab_mconv_process")


_REVERB_SPREAD = 4.65    # reverb_params: the longest line over the shortest (21.5 ms -> 100 ms)


def _primes_from(lengths):
    """Per length the smallest prime >= it that no earlier length took (ascending input: ascending, distinct output)."""
    out, last = [], 1
    for want in lengths:
        p = max(int(want), last + 1, 2)
        while any(p % d == 0 for d in range(2, int(p ** 0.5) + 1)):
            p += 1
        out.append(p)
        last = p
    return out


def reverb_params(rt60_s, rt60_hf_s=None, size_ms=21.5, lines=8, outs=2, wet_db=-6.0, dry_db=0.0, fs=48000.0,
                  delays=None):
    """(delays int32 [T][N], table float32 [T][N (3 + outs) + 1]) of ReverbPlan from the knobs of a reverb; every
    argument a scalar or an array with an entry per track (all scalars: T = 1); float64, rounded once.
    delays: unless given ([N] or [T][N]), distinct primes ascending from size_ms, the targets spread geometrically up to
    4.65 times that.  Line i of m samples gets g = 10^(-3 m / (rt60 fs)) / sqrt(N): -60 dB after rt60 seconds round the
    loop.  rt60_hf_s (<= rt60_s) is the decay time at the Nyquist frequency: with rho the ratio of the two per-pass gains,
    damp = (1 - rho) / (1 + rho), the one-pole whose Nyquist gain is rho and whose DC gain is 1; None: no damping.
    b = 1; c[o] = wet / sqrt(N) times row 1 + o of the Hadamard matrix (signs (-1)^popcount(row & i)), so the two
    outputs decorrelate; dry from dry_db.  g and damp are held to the plan's limits."""
    import numpy as np
    N, O = int(lines), int(outs)
    if N not in (4, 8, 16) or O not in (1, 2):
        raise ValueError("lines must be 4, 8 or 16 and outs 1 or 2")
    knobs = [np.atleast_1d(np.asarray(a, np.float64)) for a in
             (rt60_s, rt60_s if rt60_hf_s is None else rt60_hf_s, size_ms, wet_db, dry_db)]
    if any(a.ndim != 1 for a in knobs):
        raise ValueError("a knob is a scalar or has an entry per track")
    T = max(a.shape[0] for a in knobs)
    if delays is not None:
        delays = np.asarray(delays)
        if delays.ndim == 2:
            T = max(T, delays.shape[0])
    rt60, rt60_hf, size, wet_db, dry_db = (np.broadcast_to(a, (T,)) for a in knobs)
    if (rt60 <= 0.0).any() or (rt60_hf <= 0.0).any() or (rt60_hf > rt60).any() or (size <= 0.0).any() or fs <= 0.0:
        raise ValueError("needs rt60_s > 0, 0 < rt60_hf_s <= rt60_s, size_ms > 0, fs > 0")
    if delays is None:
        steps = _REVERB_SPREAD ** (np.arange(N, dtype=np.float64) / (N - 1))
        m = np.array([_primes_from(np.rint(size[t] * fs / 1000.0 * steps)) for t in range(T)], np.int64)
    else:
        m = np.broadcast_to(delays.astype(np.int64), (T, N))
    mf = m.astype(np.float64)
    per_pass = 10.0 ** (-3.0 * mf / (rt60[:, None] * fs))
    rho = 10.0 ** (-3.0 * mf / (rt60_hf[:, None] * fs)) / per_pass
    gmax = np.float32(lib.gab_reverb_gmax(N))
    g = np.minimum((per_pass / np.sqrt(float(N))).astype(np.float32), gmax)
    damp = np.minimum(((1.0 - rho) / (1.0 + rho)).astype(np.float32), np.float32(1.0 - 2.0 ** -20))
    i = np.arange(N)
    signs = [np.array([(-1.0) ** bin((1 + o) & int(k)).count("1") for k in i]) for o in range(O)]
    wet = 10.0 ** (wet_db / 20.0) / np.sqrt(float(N))
    c = [(wet[:, None] * s[None, :]).astype(np.float32) for s in signs]
    dry = (10.0 ** (dry_db / 20.0)).astype(np.float32)[:, None]
    table = np.concatenate([g, damp, np.ones((T, N), np.float32)] + c + [dry], axis=1).astype(np.float32)
    return np.ascontiguousarray(m.astype(np.int32)), np.ascontiguousarray(table)


class ReverbPlan(_TrackPlan, _Prepared):
    """gab_reverb_plan: a feedback delay network per track: `lines` (4, 8, 16) delay lines of integer length fed back
    through a Hadamard matrix with a damping low-pass in the loop, `outs` (1, 2) outputs per track.  Parameters per
    track {g[N], damp[N], b[N], c[outs][N], dry} (reverb_params makes them from decay times) and a delay per line; a
    new plan is pass-through; new parameters are ramped in over the next buffer unless ramp=False, new delays act from
    the next buffer.  The output is [tracks*outs][bufsize], row t*outs + o."""

    _destroy = "gab_reverb_destroy"

    def __init__(self, tracks, bufsize, lines=8, outs=2, max_delay=8192):
        self.lines, self.outs, self.max_delay = lines, outs, max_delay
        self.row_floats = lines * (3 + outs) + 1
        self._create(tracks, bufsize, lines, outs, max_delay)

    def set_params(self, table, ramp=True, first_track=None):
        """table: device tensor [tracks][row_floats], or [n][row_floats] for tracks [first_track, first_track + n).
        ramp=True: reached linearly over the next processed buffer; ramp=False: at once."""
        n = self._rows(table, self.row_floats, first_track)
        self._set("params", _dev(table), first_track, n, 1 if ramp else 0)

    def set_delays(self, delays, first_track=None):
        """delays: device int32 tensor [tracks][lines], or [n][lines] for tracks [first_track, first_track + n); they
        act from the next buffer and the lines keep their contents."""
        n = self._rows(delays, self.lines, first_track, "delays")
        self._set("delays", _dev(delays, torch.int32), first_track, n)

    def reset(self):
        """Zero lines, positions and low-pass states, current := target, a pending ramp dropped; the delays stay."""
        super().reset()

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize] -> [tracks*outs*bufsize]; out may be x itself when outs == 1."""
        return self._process("process", x, out, 1, (x.numel() * self.outs,))

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] -> [n][tracks*outs*bufsize] in one launch."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, (xs.numel() * self.outs,), n)

    def params(self):
        """Copies of (current, target), each [tracks][row_floats]."""
        return self._tables("params", self.row_floats)

    def state(self):
        """Copies of (lines [tracks][lines][capacity] float32, write positions [tracks] int64, low-pass states
        [tracks][lines] float32, delays [tracks][lines] int32)."""
        r, p, q, d, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        check(lib.gab_reverb_state(self._h, C.byref(r), C.byref(cap), C.byref(p), C.byref(q), C.byref(d)))
        T, N = self.tracks, self.lines
        ring = _view(r.value, T * N, cap.value).clone().view(T, N, cap.value)
        delays = _view(d.value, T, N).clone().view(torch.int32)
        return ring, _positions(p.value, T), _view(q.value, T, N).clone(), delays

    # prepare(x, out, stream=None): for a loop over the same buffers or a graph capture; all state that changes is on the
    # device, and which kernel form runs (steady, or the ramp form when a ramp is pending) is the host's choice at the
    # call and what a capture replays: gab_c_api.h, "Captured calls".
    launch = _launcher("gab_reverb_process")


class MeterPlan(_TrackPlan, _Prepared):
    """gab_meter_plan: one row of eight levels (FIELDS, all linear) per track and buffer, with carried state: the
    true-peak history, the weighting filter's state, the peak hold and a ring of the last `window` weighted mean
    squares.  The input is only read.  A new plan weighs with BS.1770's K curve at 48 kHz and holds its peak until
    reset."""

    _destroy = "gab_meter_destroy"
    FIELDS = ("peak", "true_peak", "ms", "kms", "peak_hold", "true_peak_max", "kms_window", "nonfinite")

    def __init__(self, tracks, bufsize, window=1):
        self.window = window
        self._create(tracks, bufsize, window)

    def set_weighting(self, sections):
        """sections: device tensor [2][5] = {b0, b1, b2, a1, a2} (a0 = 1), the same for every track; in force from
        the next buffer, the filter state is kept."""
        assert sections.numel() == 10
        check(lib.gab_meter_set_weighting(self._h, _dev(sections), _stream()))

    def set_decay(self, decay):
        """peak_hold's factor per buffer, within [0, 1]; 1 holds until reset."""
        check(lib.gab_meter_set_decay(self._h, float(decay), _stream()))

    def reset(self):
        """Every carried value zero; the weighting and the decay stay."""
        super().reset()

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize]; returns the rows [tracks][8]."""
        return self._process("process", x, out, 1, (self.tracks, len(self.FIELDS)))

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch; returns the rows [n][tracks][8]."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, (n, self.tracks, len(self.FIELDS)), n)

    def state(self):
        """Copies of (hist [tracks][16] = the last 11 samples, peak_hold, true_peak_max, 3 zeros; filter
        [tracks][2][2] = (s1, s2) per section; ring [tracks][window]; pos [tracks] int64)."""
        h, f, r, p = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib.gab_meter_state(self._h, C.byref(h), C.byref(f), C.byref(r), C.byref(p)))
        return (_view(h.value, self.tracks, 16).clone(), _view(f.value, self.tracks, 4).clone().view(self.tracks, 2, 2),
                _view(r.value, self.tracks, self.window).clone(), _positions(p.value, self.tracks))

    launch = _launcher("gab_meter_process")


class ResamplePlan(_TrackPlan):
    """gab_resample_plan: every track's stream from one sample rate to another by up / down (reduced by their gcd), a
    polyphase FIR of `ntaps` taps per phase with carried history and an exact carried position.  A buffer of `bufsize`
    input samples gives floor or ceil of bufsize * up / down output samples; `out_capacity` is the ceil, and the rest
    of a row is zeros.  The counts are host integers; the pattern repeats every `period` buffers.  (No prepare():
    the position is a launch argument, so a captured process replays one position.)"""

    _destroy = "gab_resample_destroy"

    def __init__(self, tracks, bufsize, up, down, taps=None):
        if taps is None:
            taps = self.default_taps(up, down)
        self._create(tracks, bufsize, up, down, taps)
        v = [C.c_int(0) for _ in range(5)]
        check(lib.gab_resample_shape(self._h, *[C.byref(c) for c in v]))
        self.up, self.down, self.ntaps, self.out_capacity, self.period = (c.value for c in v)
        self.latency = self.ntaps // 2          # input samples

    @staticmethod
    def default_taps(up, down):
        """The smallest multiple of 8 that is at least 32 * max(1, down / up)."""
        import math
        g = math.gcd(up, down)
        L, M = up // g, down // g
        return 8 * -(-(32 * max(L, M)) // (8 * L))

    @staticmethod
    def counts(bufsize, up, down, first_buffer, n):
        """The output counts of buffers first_buffer .. first_buffer + n - 1 since a reset: host integers, no GPU."""
        import math
        g = math.gcd(up, down)
        L, M = up // g, down // g
        lo = [-(-(k * bufsize * L) // M) for k in range(first_buffer, first_buffer + n + 1)]
        return [b - a for a, b in zip(lo, lo[1:])]

    def reset(self):
        """Zero history, position 0; the taps stay."""
        super().reset()

    def set_taps(self, t):
        """t: device tensor [up][ntaps]; in force from the next buffer, history and position are kept."""
        assert t.numel() == self.up * self.ntaps
        check(lib.gab_resample_set_taps(self._h, _dev(t), _stream()))

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize]; returns (out [tracks][out_capacity], n_out): the first n_out
        elements of every row are samples, the rest zeros."""
        n = C.c_int(0)
        return self._process("process", x, out, 1, (self.tracks, self.out_capacity), C.byref(n)), n.value

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch; returns (out [n][tracks][out_capacity], counts)."""
        n = _n_buffers(self, xs)
        counts = (C.c_int * max(n, 1))()
        out = self._process("process_batch", xs, out, n, (n, self.tracks, self.out_capacity), n, counts)
        return out, list(counts[:n])

    def _state(self):
        h, t, k = C.c_void_p(), C.c_void_p(), C.c_longlong(0)
        check(lib.gab_resample_state(self._h, C.byref(h), C.byref(t), C.byref(k)))
        return h.value, t.value, k.value

    def taps(self):
        """A copy of the table in force, [up][ntaps]."""
        return _view(self._state()[1], self.up, self.ntaps).clone()

    def state(self):
        """(a copy of hist [tracks][ntaps-1] = the last ntaps-1 input samples, oldest first; buffers since the reset
        mod period)."""
        h, _, k = self._state()
        return _view(h, self.tracks, self.ntaps - 1).clone(), k


def spectrum_band_edges(bands, fs=48000.0, fmin=20.0, fmax=None):
    """bands + 1 bin edges for SpectrumPlan.set_bands, logarithmically spaced from fmin to fmax (default fs / 2) on
    the 1024-point grid of fs / 1024 Hz a bin: a fractional-octave display.  Edge b is the bin nearest
    fmin (fmax / fmin) ** (b / bands), and the table is then made strictly increasing inside [0, 513]: low bands, where
    the spacing is below a bin, take one bin each."""
    if not 1 <= bands <= 64:
        raise ValueError("bands must be 1..64")
    fmax = fs / 2.0 if fmax is None else fmax
    if not (0.0 < fmin < fmax <= fs / 2.0):
        raise ValueError("needs 0 < fmin < fmax <= fs / 2")
    e = [int(round(fmin * (fmax / fmin) ** (b / bands) * 1024.0 / fs)) for b in range(bands + 1)]
    e[bands] += 1                                     # fmax's bin belongs to the last band
    for b in range(1, bands + 1):                     # strictly increasing, upwards
        e[b] = max(e[b], e[b - 1] + 1)
    e[bands] = min(e[bands], 513)
    for b in range(bands - 1, -1, -1):                # and back down below the ceiling
        e[b] = min(e[b], e[b + 1] - 1)
    assert e[0] >= 0
    return e


class _StftPlan(_TrackPlan):
    """What the short-time Fourier plans (spectrum, resynthesis, denoise) share: frames of N samples, rows of BINS
    complex bins, on the grid of `hop` samples since the reset."""

    N = 1024
    BINS = 513

    def _create(self, tracks, bufsize, hop, *rest):
        self.hop = hop
        super()._create(tracks, bufsize, hop, *rest)

    @staticmethod
    def counts(bufsize, hop, first_buffer, n):
        """The frame counts of buffers first_buffer .. first_buffer + n - 1 since a reset: host integers, no GPU."""
        lo = [(k * bufsize) // hop for k in range(first_buffer, first_buffer + n + 1)]
        return [b - a for a, b in zip(lo, lo[1:])]

    def _streams_out(self):
        """Of the plans that write a stream: its `latency`, and what a call that takes no frame points at."""
        c = C.c_int(0)
        check(self._fn("latency")(self._h, C.byref(c)))
        self.latency = c.value                              # samples
        self._none = torch.zeros(2, dtype=torch.float32, device="cuda")

    def _refuse_moving_grid(self):
        """prepare() only where hop divides bufsize: the frame phase and the count are launch arguments, constant there
        (phase 0, bufsize / hop frames a call) and nowhere else."""
        if self.bufsize % self.hop:
            raise ValueError("%s.prepare: hop %d does not divide bufsize %d, so the frame phase and the "
                             "frame count change from call to call and a prepared or captured call would repeat one "
                             "of them" % (type(self).__name__, self.hop, self.bufsize))


class SpectrumPlan(_StftPlan):
    """gab_spec_plan: a short-time Fourier analyser per track.  Frames of 1024 samples every `hop` samples of the
    stream (the last 1023 samples are carried), under a window (a new plan: periodic Hann), as complex bins
    (mode="complex": rows [frames][tracks][513][2]), as powers per bin (mode="power": [frames][tracks][513]; a sine of
    amplitude A on a bin reads A * A) or as powers per band (bands 1..64: [frames][tracks][bands]).  A call emits the
    frames that end inside it, possibly none; `counts` says how many without a GPU."""

    _destroy = "gab_spec_destroy"
    MODES = {"complex": 0, "power": 1}

    def __init__(self, tracks, bufsize, hop=512, mode="power", bands=0):
        if mode not in self.MODES:
            raise ValueError("mode must be 'complex' or 'power'")
        self.mode, self.bands = mode, bands
        self._create(tracks, bufsize, hop, self.MODES[mode], bands)
        self.row_shape = (self.BINS, 2) if mode == "complex" else (bands or self.BINS,)

    def frames(self, n_buffers=1):
        """The largest frame count a call of n_buffers buffers can return: the rows an `out` must hold."""
        c = C.c_int(0)
        check(lib.gab_spec_frames(self._h, n_buffers, C.byref(c)))
        return c.value

    def reset(self):
        """Zero history, position 0; the window and the band edges stay."""
        super().reset()

    def set_window(self, w):
        """w: device tensor [1024], the same for every track; every value finite and the sum not zero.  In force from
        the next call, the history is kept."""
        assert w.numel() == self.N
        check(lib.gab_spec_set_window(self._h, _dev(w), _stream()))

    def set_bands(self, edges):
        """edges: bands + 1 host integers, 0 <= e_0 < e_1 < ... < e_bands <= 513 (spectrum_band_edges makes them)."""
        edges = [int(e) for e in edges]
        if len(edges) != self.bands + 1:
            raise ValueError("edges must hold bands + 1 = %d integers" % (self.bands + 1))
        check(lib.gab_spec_set_bands(self._h, (C.c_int * len(edges))(*edges)))

    def _rows_out(self, out, n):
        cap = self.frames(n)
        if out is None:
            out = torch.empty((cap, self.tracks) + self.row_shape, dtype=torch.float32, device="cuda")
        assert out.numel() >= cap * self.tracks * torch.Size(self.row_shape).numel()
        return out, cap

    def _cut(self, out, frames):
        return out.view(-1, self.tracks, *self.row_shape)[:frames]

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize]; returns the rows of the frames that ended in it,
        [frames][tracks][...] (a view of `out`, or of a new tensor of frames(1) rows), possibly [0]."""
        out, _ = self._rows_out(out, 1)
        f = C.c_int(0)
        self._process("process", x, out, 1, None, C.byref(f), sized=False)
        return self._cut(out, f.value)

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one call; returns the rows of the frames that ended in them."""
        n = _n_buffers(self, xs)
        out, _ = self._rows_out(out, n)
        f = C.c_int(0)
        self._process("process_batch", xs, out, n, None, n, C.byref(f), sized=False)
        return self._cut(out, f.value)

    def state(self):
        """(a copy of hist [tracks][1023] = the last 1023 samples, oldest first; a copy of the window [1024]; samples
        since the reset mod hop)."""
        h, w, p = C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib.gab_spec_state(self._h, C.byref(h), C.byref(w), C.byref(p)))
        return _view(h.value, self.tracks, self.N - 1).clone(), _view(w.value, 1, self.N).clone().view(self.N), p.value

    def prepare(self, x, out, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  Only where hop divides bufsize: the frame phase and the count are launch arguments, constant
        there (phase 0, bufsize / hop frames a call) and nowhere else."""
        self._refuse_moving_grid()
        assert out.numel() >= self.frames(1) * self.tracks * torch.Size(self.row_shape).numel()
        self._n = C.c_int(0)
        return (self._h, _dev(x), _dev(out), C.byref(self._n), _stream(stream))

    launch = _launcher("gab_spec_process")


def synthesis_window(w, hop):
    """The least-squares dual of an analysis window w [1024] at `hop`, for ResynthesisPlan.set_window:
    g[n] = w[n] / sum_m w[n + m hop]^2, m over every index inside 0..1023 in ascending order, 0 where that sum is 0; in
    float64 on w's values, rounded once to float32.  Then sum_j w g = 1 on the hop grid, and SpectrumPlan (window w) ->
    ResynthesisPlan (window g) returns the stream delayed by 1024 samples.  A float32 tensor on w's device (the CPU for
    anything that is not a tensor).  The dual is ill-conditioned as hop approaches 1024, where frames overlap only in
    the window's skirts: for the periodic Hann window the largest |g| is 0.67 / 1.2 / 2.6 / 430 / 1e5 at hop 256 / 512 /
    700 / 1000 / 1023, and at hop 1024 the window's zero at n = 0 cannot be undone."""
    if not 32 <= hop <= 1024:
        raise ValueError("hop must be 32..1024")
    device = w.device if isinstance(w, torch.Tensor) else "cpu"
    w64 = torch.as_tensor(w).detach().to("cpu", torch.float64).reshape(-1)
    if w64.numel() != 1024:
        raise ValueError("the window must hold 1024 values")
    sq, den = w64 * w64, torch.zeros(hop, dtype=torch.float64)
    for m in range(0, 1024, hop):                         # ascending index, one addition each
        seg = sq[m:m + hop]
        den[:seg.numel()] += seg
    den = den.repeat(-(-1024 // hop))[:1024]
    g = torch.where(den == 0, torch.zeros_like(w64), w64 / torch.where(den == 0, torch.ones_like(den), den))
    return g.to(torch.float32).to(device)


class ResynthesisPlan(_StftPlan):
    """gab_resyn_plan: the overlap-add inverse of SpectrumPlan(mode="complex").  Rows [frames][tracks][513][2] become
    the stream again: every frame is inverse-transformed, multiplied by the synthesis window (a new plan: the dual of
    the periodic Hann window at `hop`, see synthesis_window) and added on the hop grid in a fixed order; the 1024 samples
    later frames still add to are carried on the device.  The output is the resynthesised stream delayed by `latency` =
    1024 samples, whatever the cut.  A call of n buffers takes exactly the `count(n)` frames that a SpectrumPlan of the
    same bufsize and hop emits for the same call, possibly none; `counts` says how many without a GPU."""

    _destroy = "gab_resyn_destroy"

    def __init__(self, tracks, bufsize, hop=512):
        self._create(tracks, bufsize, hop)
        self._streams_out()

    def frames(self, n_buffers=1):
        """The largest frame count a call of n_buffers buffers can take."""
        c = C.c_int(0)
        check(lib.gab_resyn_frames(self._h, n_buffers, C.byref(c)))
        return c.value

    def count(self, n_buffers=1):
        """The frame count the NEXT call of n_buffers buffers takes; the plan does not move."""
        c = C.c_int(0)
        check(lib.gab_resyn_count(self._h, n_buffers, C.byref(c)))
        return c.value

    def reset(self):
        """Zero accumulator, position 0; the window stays."""
        super().reset()

    def set_window(self, g):
        """g: device tensor [1024], the same for every track; every value finite.  Acts on the frames of the next
        call; what is in the accumulator stays."""
        assert g.numel() == self.N
        check(lib.gab_resyn_set_window(self._h, _dev(g), _stream()))

    def _rows_in(self, rows, n, who):
        f = self.count(n)
        if rows.numel() != f * self.tracks * self.BINS * 2:
            raise ValueError("ResynthesisPlan.%s: this call takes exactly %d frames of [%d][513][2] values, rows holds "
                             "%d values" % (who, f, self.tracks, rows.numel()))
        return _dev(rows) if f else _dev(self._none)

    def _run(self, what, rows, out, n, *rest):
        ptr = self._rows_in(rows, n, what)
        shape = (self.tracks, self.bufsize) if n == 1 and not rest else (n, self.tracks, self.bufsize)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device="cuda")
        assert out.numel() == n * self.tracks * self.bufsize
        f = C.c_int(0)
        check(self._fn(what)(self._h, ptr, _dev(out), *rest, C.byref(f), _stream()))
        return out

    def process(self, rows, out=None):
        """One buffer: rows [count(1)][tracks][513][2] in, the next bufsize samples of every track out,
        [tracks][bufsize] (`out`, or a new tensor)."""
        return self._run("process", rows, out, 1)

    def process_batch(self, rows, n_buffers, out=None):
        """n_buffers consecutive buffers in one call: rows [count(n_buffers)][tracks][513][2] in, [n_buffers][tracks]
        [bufsize] out."""
        return self._run("process_batch", rows, out, n_buffers, n_buffers)

    def state(self):
        """(a copy of acc [tracks][1024]: acc[i] the partial sum of the output sample i places behind the position; a
        copy of the window [1024]; samples since the reset mod hop)."""
        a, w, p = C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib.gab_resyn_state(self._h, C.byref(a), C.byref(w), C.byref(p)))
        return _view(a.value, self.tracks, self.N).clone(), _view(w.value, 1, self.N).clone().view(self.N), p.value

    def prepare(self, rows, out, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  Only where hop divides bufsize: the frame phase and the count are launch arguments, constant
        there (phase 0, bufsize / hop frames a call) and nowhere else."""
        self._refuse_moving_grid()
        assert rows.numel() == (self.bufsize // self.hop) * self.tracks * self.BINS * 2
        assert out.numel() == self.tracks * self.bufsize
        self._n = C.c_int(0)
        return (self._h, _dev(rows), _dev(out), C.byref(self._n), _stream(stream))

    launch = _launcher("gab_resyn_process")


def denoise_params(floor_db=-24.0, attack_ms=5.0, release_ms=80.0, hop=256, fs=48000.0):
    """A row (all arguments scalars) or a table [n][3] float32 of DenoisePlan parameters {floor, att, rel} from the knobs
    of a noise reduction; float64, rounded once.  floor = 10^(floor_db / 20) is the gain of a shut bin (floor_db <= 0;
    -inf shuts it completely); att and rel are per FRAME, exp(-hop / (fs t)) for the time constant t of an opening and
    of a closing bin, and a time of 0 is a coefficient of 0 (the gain jumps)."""
    import numpy as np
    args = [np.asarray(a, np.float64) for a in (floor_db, attack_ms, release_ms)]
    scalar = all(a.ndim == 0 for a in args)
    floor_db, att_ms, rel_ms = np.broadcast_arrays(*[np.atleast_1d(a) for a in args])
    if (floor_db > 0.0).any() or (att_ms < 0.0).any() or (rel_ms < 0.0).any() or fs <= 0.0 or hop <= 0:
        raise ValueError("needs floor_db <= 0, attack_ms and release_ms >= 0, fs > 0 and hop > 0")
    att = np.where(att_ms > 0.0, np.exp(-hop / (fs * np.where(att_ms > 0.0, att_ms / 1000.0, 1.0))), 0.0)
    rel = np.where(rel_ms > 0.0, np.exp(-hop / (fs * np.where(rel_ms > 0.0, rel_ms / 1000.0, 1.0))), 0.0)
    table = np.stack([10.0 ** (floor_db / 20.0), att, rel], axis=-1).astype(np.float32)
    return table[0] if scalar else table


def denoise_thresholds(power_rows, sensitivity_db=6.0):
    """The "learn a noise profile" step: power_rows [frames][tracks][513] of SpectrumPlan(mode="power"), recorded over a
    stretch of noise alone, become DenoisePlan thresholds [tracks][513]: the float64 mean over the frames times
    10^(sensitivity_db / 10), rounded once to float32.  A tensor on power_rows' device (a numpy array for anything that
    is not a tensor)."""
    import numpy as np
    is_tensor = isinstance(power_rows, torch.Tensor)
    p = (power_rows.detach().to("cpu").numpy() if is_tensor else np.asarray(power_rows)).astype(np.float64)
    if p.ndim != 3 or p.shape[0] == 0 or p.shape[2] != 513:
        raise ValueError("power_rows must be [frames][tracks][513] with at least one frame")
    thr = (p.mean(axis=0) * 10.0 ** (float(sensitivity_db) / 10.0)).astype(np.float32)
    return torch.from_numpy(thr).to(power_rows.device) if is_tensor else thr


class DenoisePlan(_StftPlan):
    """gab_dn_plan: a spectral noise gate per (track, bin) with a smoothed gain.  process / process_batch take the stream
    and return it gated and delayed by `latency` = 1024 samples in ONE launch: SpectrumPlan(mode="complex")'s analysis,
    the gate, ResynthesisPlan's overlap-add, bit for bit that composition.  process_rows is the gate alone, complex rows
    [frames][tracks][513][2] in and out, for rows one already holds; it moves the mask only.  Tables: thresholds
    [tracks][513] on the power of a bin (denoise_thresholds learns them from noise) and {floor, att, rel} per track
    (denoise_params).  A new plan is transparent."""

    _destroy = "gab_dn_destroy"
    FIELDS = ("floor", "att", "rel")

    def __init__(self, tracks, bufsize, hop=256):
        self._create(tracks, bufsize, hop)
        self._streams_out()

    def reset(self):
        """Zero history and accumulator, a mask of ones, position 0; the tables and the windows stay."""
        super().reset()

    def set_thresholds(self, thr, first_track=0):
        """thr: device tensor [n][513] for tracks [first_track, first_track + n): every value >= 0 or +inf (always
        shut).  Acts from the next frame processed; the mask is kept."""
        n = self._rows(thr, self.BINS, first_track, "thr")
        check(lib.gab_dn_set_thresholds(self._h, _dev(thr), first_track, n, _stream()))

    def set_params(self, rows, first_track=0):
        """rows: device tensor [n][3] of {floor, att, rel} for tracks [first_track, first_track + n): 0 <= floor <= 1,
        0 <= att < 1, 0 <= rel < 1.  Acts from the next frame processed, unramped; the mask is kept."""
        n = self._rows(rows, len(self.FIELDS), first_track, "rows")
        check(lib.gab_dn_set_params(self._h, _dev(rows), first_track, n, _stream()))

    def set_windows(self, w, g):
        """w, g: device tensors [1024], the analysis and the synthesis window, the same for every track; every value
        finite and w's sum not zero (synthesis_window makes g from w).  A refused set keeps both."""
        assert w.numel() == self.N and g.numel() == self.N
        check(lib.gab_dn_set_windows(self._h, _dev(w), _dev(g), _stream()))

    def process(self, x, out=None):
        """One buffer, track-major [tracks*bufsize] in, the next bufsize samples of every track out (`out`, or a new
        tensor like x); x and out may not overlap."""
        return self._process("process", x, out, 1, None)

    def process_batch(self, xs, out=None):
        """Consecutive buffers [n][tracks*bufsize] in one launch, [n][tracks][bufsize] both ways."""
        n = _n_buffers(self, xs)
        return self._process("process_batch", xs, out, n, None, n)

    def process_rows(self, rows, out=None):
        """The gate alone on rows [frames][tracks][513][2] (any number of frames, none too): returns the gated rows in
        `out` (rows itself for in place; None: a new tensor).  Moves the mask, nothing else."""
        f, rest = divmod(rows.numel(), self.tracks * self.BINS * 2)
        if rest:
            raise ValueError("DenoisePlan.process_rows: rows must hold whole frames of [%d][513][2] values" % self.tracks)
        out = torch.empty_like(rows) if out is None else out
        assert out.numel() == rows.numel()
        a, b = (_dev(rows), _dev(out)) if f else (_dev(self._none), _dev(self._none))
        check(lib.gab_dn_process_rows(self._h, a, b, f, _stream()))
        return out

    def state(self):
        """Copies of (hist [tracks][1023], the last 1023 samples oldest first; acc [tracks][1024], the partial sums
        behind the position; mask [tracks][513]; samples since the reset mod hop)."""
        h, a, m, p = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        check(lib.gab_dn_state(self._h, C.byref(h), C.byref(a), C.byref(m), C.byref(p)))
        return (_view(h.value, self.tracks, self.N - 1).clone(), _view(a.value, self.tracks, self.N).clone(),
                _view(m.value, self.tracks, self.BINS).clone(), p.value)

    def tables(self):
        """Copies of (thr [tracks][513], params [tracks][3])."""
        t, p = C.c_void_p(), C.c_void_p()
        check(lib.gab_dn_tables(self._h, C.byref(t), C.byref(p)))
        return _view(t.value, self.tracks, self.BINS).clone(), _view(p.value, self.tracks, len(self.FIELDS)).clone()

    def prepare(self, x, out, stream=None):
        """The ctypes arguments of process(), built once for a loop over the same buffers or a graph capture;
        `launch(args)`.  Only where hop divides bufsize: the frame phase and the count are launch arguments, constant
        there (phase 0, bufsize / hop frames a call) and nowhere else."""
        self._refuse_moving_grid()
        assert x.numel() == out.numel() == self.tracks * self.bufsize
        return (self._h, _dev(x), _dev(out), _stream(stream))

    launch = _launcher("gab_dn_process")


def fdtd_default_params(nx, ny=None, nz=None):
    P = FdtdParams()
    check(lib.gab_fdtd_default_params(nx, nx if ny is None else ny, nx if nz is None else nz,
                                      C.byref(P)))
    return P


FDTD_FORMS = ("resident", "sample_tile", "lds_32x8", "lds_32x16", "lds_64x4", "lds_64x8", "step_vec4", "step_scalar")


class FdtdPlan(_Handle):
    _destroy = "gab_fdtd_destroy"

    def __init__(self, params):
        self.params = params
        self._h = C.c_void_p()
        check(lib.gab_fdtd_create(C.byref(self._h), C.byref(params)))

    def reset(self):
        check(lib.gab_fdtd_reset(self._h, _stream()))

    def process(self, x, out, tracks, bufsize, first_sample, n_samples):
        check(lib.gab_fdtd_process(self._h, _dev(x), _dev(out), tracks, bufsize, first_sample,
                                   n_samples, _stream()))
        return out

    def set_form(self, form):
        """"auto" (resident in LDS where the room fits) or "step" (one launch per step): gab_fdtd_set_form."""
        check(lib.gab_fdtd_set_form(self._h, {"auto": 0, "step": 1}[form]))

    def form(self, tracks, n_samples, capturing=False):
        """(kernel form by name (FDTD_FORMS), True if through the plan's graph cache) of a process() call of n_samples:
        gab_debug_fdtd_form."""
        form, graph = C.c_int(0), C.c_int(0)
        check(lib.gab_debug_fdtd_form(self._h, tracks, n_samples, 1 if capturing else 0, C.byref(form), C.byref(graph)))
        return FDTD_FORMS[form.value], bool(graph.value)

    def status(self):
        """Synchronises the current stream; raises GabError if the last process() call's resident launch
        gave up waiting for a neighbour workgroup: gab_fdtd_status."""
        check(lib.gab_fdtd_status(self._h, _stream()))

    def resident(self):
        """(takes the LDS-resident whole-buffer kernel, its workgroups): gab_fdtd_resident."""
        r, w = C.c_int(0), C.c_int(0)
        check(lib.gab_fdtd_resident(self._h, C.byref(r), C.byref(w)))
        return bool(r.value), w.value

    def set_track_positions(self, src_xyz, rcv_xyz):
        """Per-track source and receiver cells: two (tracks, 3) integer arrays of (x, y, z);
        pass None, None to return to the shared cells of the params."""
        import numpy as np
        if src_xyz is None:
            check(lib.gab_fdtd_set_track_positions(self._h, None, None, 0))
            return
        src = np.ascontiguousarray(src_xyz, np.int32)
        rcv = np.ascontiguousarray(rcv_xyz, np.int32)
        if src.ndim != 2 or src.shape[1] != 3 or rcv.shape != src.shape:
            raise ValueError("positions must be two (tracks, 3) arrays")
        ip = C.POINTER(C.c_int)
        check(lib.gab_fdtd_set_track_positions(self._h, src.ctypes.data_as(ip), rcv.ctypes.data_as(ip),
                                               src.shape[0]))

    def pressure(self):
        """A copy of the pressure grid as a torch tensor (nz, ny, nx)."""
        P = self.params
        out = torch.empty(P.nx * P.ny * P.nz, dtype=torch.float32, device="cuda")
        check(lib.gab_fdtd_copy_pressure(self._h, _dev(out), _stream()))
        return out.view(P.nz, P.ny, P.nx)
