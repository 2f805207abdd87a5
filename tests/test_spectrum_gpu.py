"""The spectrum plan (gab_spec_*, SpectrumPlan) on the device, against spectrum_twin.py.

The transform is held by a bound, per track and frame: max_k |X - X64| / (peak_t + peak_p) <= min(FACTOR c_twin, 1e-5),
c_twin the twin's figure on the same frames.  Everything around the transform is exact: the framing (the same stream
gives the same frames however it is cut, batched, aligned or hopped), the powers (numpy float32 on the kernel's complex
bits), the bands (the ordered float32 sum of the kernel's powers), the carried history, and the isolation of a pair.
Track counts 1, 2, 3, 9, 17: an odd last track, and the crossing of the eight-track workgroup.  Streams of at most 4096
samples."""
import ctypes

import numpy as np
import pytest

import conv_pair_twin as tw
import spectrum_twin as st
from test_conv_plan_state_gpu import dev, gab, host, same_bits  # noqa: F401
from test_fft_levels_gpu import KNOWN_FACTOR

pytestmark = pytest.mark.gpu

TRACKS = [1, 2, 3, 9, 17]
N, BINS, HIST = st.N, st.BINS, st.HIST
TOTAL = 4096
# The project's own factor for this transform (test_fft_levels_gpu.held).  Measured on Hann frames of these streams:
# 2.34 to 3.13 (profiles/r22_spectrum.txt); one-hot windows 0.0 to 3.0, under KNOWN_FACTOR.
FACTOR = 4.0
CUTS = (64, 100, 512, 1536)

_streams = {}


def stream(T):
    """The shared input of track count T: [T, 4096] at conv_pair_twin.levels(T), made once and never changed."""
    if T not in _streams:
        x = st.noise(T, TOTAL, seed=100 + T)
        x.setflags(write=False)
        _streams[T] = x
    return _streams[T]


def off_by_4_bytes(a):
    """The same values in device memory 4 bytes past a 16-byte boundary."""
    import torch
    t = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[1:].copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
    v = t[1:]
    assert v.data_ptr() % 16 == 4
    return v


def run(plan, x, batch=None, put=dev, after=None):
    """The rows of every whole buffer of x [T, total] through `plan`: per buffer (batch None) or `batch` buffers a
    call.  Returns (rows [F, T, ...], the count of every call).  after(plan, samples so far) runs behind every call."""
    import torch
    T, B = plan.tracks, plan.bufsize
    n = x.shape[1] // B
    bl = st.blocks(x[:, :n * B], B)
    out, calls, i = [], [], 0
    while i < n:
        if batch is None:
            r = plan.process(put(bl[i]))
            i += 1
        else:
            r = plan.process_batch(put(bl[i:i + batch]))
            i += min(batch, n - i)
        calls.append(r.shape[0])
        out.append(r.clone())
        if after is not None:
            after(plan, i * B)
    return host(torch.cat(out)), calls


def cplx(rows):
    rows = rows.astype(np.float64)
    return rows[..., 0] + 1j * rows[..., 1]


def hist_is_the_streams_tail(plan, x, p, H):
    h, _, phase = plan.state()
    want = np.zeros((x.shape[0], HIST), np.float32)
    k = min(p, HIST)
    want[:, HIST - k:] = x[:, p - k:p]
    assert same_bits(host(h), want), p
    assert phase == p % H


# ---- accuracy --------------------------------------------------------------------------------------------------------
def twin_side(x, H, w):
    frames = st.windowed(x, st.frame_ends(0, x.shape[1], H), w)
    X64 = st.truth(frames)
    c, level = st.figures(st.spectra(frames), X64)
    return X64, tw.c_max(c), level


@pytest.mark.parametrize("T", TRACKS)
def test_every_track_and_frame_is_within_4_c_twin_of_its_pairs_peak(gab, T):
    x = stream(T)
    X64, c_twin, level = twin_side(x, 512, st.window_hann())
    plan = gab.SpectrumPlan(T, 512, 512, "complex")
    rows, _ = run(plan, x)
    plan.close()
    cg, _ = st.figures(cplx(rows), X64)
    print("\nspectrum hann T %d c_twin %.3g c_gpu %.3g ratio %.2f" % (T, c_twin, tw.c_max(cg), tw.c_max(cg) / c_twin))
    assert 0 < c_twin <= 1e-6 and (level > 0).all()
    assert (cg <= min(FACTOR * c_twin, 1e-5)).all(), cg.max() / c_twin


ONE_HOT = (0, 1, 511, 1023)
_one_hot = {}


def one_hot_case(n0):
    """(x, ends, X64, level) of the one-hot window at n0, and c_twin: the twin's largest figure over the four windows
    (one figure for the set, as test_fft_levels_gpu's known answers share one over their impulses: the twin's
    transform is exact on an impulse at n = 0 and nearly so at n = 1, where the kernel loses what it loses anywhere)."""
    if not _one_hot:
        for m in ONE_HOT:
            x = st.noise(9, 2000, seed=20 + m, lv=np.ones(9))
            ends = st.frame_ends(0, 2000, 96)
            frames = st.windowed(x, ends, st.one_hot(m))
            X64 = st.truth(frames)
            c, level = st.figures(st.spectra(frames), X64)
            _one_hot[m] = (x, ends, X64, level, float(np.nanmax(c)))
    return _one_hot[n0][:4] + (max(v[4] for v in _one_hot.values()),)


@pytest.mark.parametrize("n0", ONE_HOT)
def test_one_hot_windows_give_the_sample_times_a_unit_phasor(gab, n0):
    """The framing's known answer: under a one-hot window at n0 frame j is x[jH - N + n0] exp(-2 pi i k n0 / N).  Held
    to float64 under KNOWN_FACTOR c_twin (an impulse's spectrum is the bare product of the passes' twiddles:
    test_fft_levels_gpu.KNOWN_FACTOR) and to the closed form within 4e-6 of the pair's peak."""
    T, B, H = 9, 100, 96
    x, ends, X64, level, c_twin = one_hot_case(n0)
    plan = gab.SpectrumPlan(T, B, H, "complex")
    plan.set_window(dev(st.one_hot(n0)))
    rows, calls = run(plan, x)
    plan.close()
    assert calls == st.counts(B, H, 0, 20)
    X = cplx(rows)
    live = level > 0                                       # frames that reach back past sample 0 pick a zero
    assert live[ends.index(1056):].all() and not X[~live].any()
    err = np.abs(X - X64).max(axis=-1)
    print("\nspectrum one-hot %d c_twin %.3g ratio %.2f" % (n0, c_twin, (err[live] / level[live]).max() / c_twin))
    assert 0 < c_twin <= 1e-6
    assert (err[live] <= min(KNOWN_FACTOR * c_twin, 1e-5) * level[live]).all()
    assert (np.abs(X - st.one_hot_answer(x, ends, n0)).max(axis=-1) <= 4e-6 * level).all()


@pytest.mark.parametrize("T", TRACKS)
def test_powers_are_within_the_bound_that_follows_from_the_complex_one(gab, T):
    """|P - P64| <= inv_k (2 |X64| d + d^2) + 2^-22 P64, d the complex bound times the pair's level: the error of
    |X|^2 for an X within d, and three float32 roundings."""
    x = stream(T)
    w = st.window_hann()
    X64, c_twin, level = twin_side(x, 512, w)
    ik = st.inv_k(st.window_sum(w)).astype(np.float64)
    P64 = np.abs(X64) ** 2 * ik
    d = (min(FACTOR * c_twin, 1e-5) * level)[..., None]
    plan = gab.SpectrumPlan(T, 512, 512, "power")
    rows, _ = run(plan, x)
    plan.close()
    bound = ik * (2 * np.abs(X64) * d + d * d) + 2.0 ** -22 * P64
    assert (np.abs(rows.astype(np.float64) - P64) <= bound).all()


# ---- exact: the cut, the batch, the alignment, the hop -------------------------------------------------------------
@pytest.mark.parametrize("T", TRACKS)
@pytest.mark.parametrize("H", [256, 96])
def test_the_same_stream_gives_the_same_frames_however_it_is_cut(gab, T, H):
    x = stream(T)
    ref = gab.SpectrumPlan(T, 512, H, "complex")
    want, _ = run(ref, x)
    ref.close()
    assert want.shape == (TOTAL // H, T, BINS, 2)
    for B in CUTS:
        n = TOTAL // B
        frames = n * B // H
        for batch, put in ((None, dev), (3, dev), (n, dev), (None, off_by_4_bytes), (5, off_by_4_bytes)):
            plan = gab.SpectrumPlan(T, B, H, "complex")
            got, calls = run(plan, x, batch, put)
            plan.close()
            m = 1 if batch is None else batch
            assert calls == [st.count(k * B, min(m, n - k) * B, H) for k in range(0, n, m)], (B, batch)
            assert got.shape[0] == frames and same_bits(got, want[:frames]), (B, batch)


@pytest.mark.parametrize("T", [3, 17])
@pytest.mark.parametrize("mode,bands", [("complex", 0), ("power", 0), ("power", 31)])
def test_every_second_frame_at_hop_256_is_a_frame_at_hop_512(gab, T, mode, bands):
    x = stream(T)
    a, b = gab.SpectrumPlan(T, 512, 256, mode, bands), gab.SpectrumPlan(T, 512, 512, mode, bands)
    fine, _ = run(a, x)
    coarse, _ = run(b, x, batch=8)
    a.close()
    b.close()
    assert fine.shape[0] == 16 and coarse.shape[0] == 8
    assert same_bits(fine[1::2], coarse)


@pytest.mark.parametrize("T", [2, 3, 9])
def test_bins_are_the_power_arithmetic_on_the_complex_bits_and_bands_their_ordered_sum(gab, T):
    x = stream(T)
    B, H = 512, 256
    S = st.window_sum(st.window_hann())
    c = gab.SpectrumPlan(T, B, H, "complex")
    X, _ = run(c, x)
    c.close()
    p = gab.SpectrumPlan(T, B, H, "power")
    P, _ = run(p, x, batch=2)
    p.close()
    assert P.shape == (16, T, BINS) and same_bits(P, st.powers(X, S))
    cases = [(1, None), (31, gab.spectrum_band_edges(31)), (64, None), (4, [3, 4, 100, 500, 512]), (2, [511, 512, 513])]
    for bands, edges in cases:
        plan = gab.SpectrumPlan(T, B, H, "power", bands)
        if edges is not None:
            plan.set_bands(edges)
        got, _ = run(plan, x)
        plan.close()
        e = st.default_edges(bands) if edges is None else edges
        assert got.shape == (16, T, bands) and same_bits(got, st.band_sums(P, e)), (bands, edges)


# ---- history and shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,total", [(64, 256, 2048), (100, 96, 2000), (1536, 1024, 3072), (1, 32, 70), (7, 1000, 2100)])
def test_the_history_after_every_call_is_the_streams_tail(gab, B, H, total):
    import torch
    T = 3
    x = stream(T)[:, :total]
    want = st.spectra(st.windowed(x, st.frame_ends(0, total, H), st.window_hann()))
    plan = gab.SpectrumPlan(T, B, H, "complex")
    assert plan.frames(1) == st.capacity(B, H, 1) and plan.frames(7) == st.capacity(B, H, 7)
    hist_is_the_streams_tail(plan, x, 0, H)
    rows, calls = run(plan, x, after=lambda p, done: hist_is_the_streams_tail(p, x, done, H))
    assert calls == st.counts(B, H, 0, total // B)
    assert rows.shape[0] == total // H
    if rows.shape[0]:
        level = np.abs(want).max(axis=-1).max()
        assert np.abs(cplx(rows) - want).max() <= 1e-5 * level
    # the same stream again into the caller's rows: a call writes the rows of its frames and no other, so a call that
    # emits no frame (most calls where B < H) leaves them all alone
    plan.reset()
    hist_is_the_streams_tail(plan, x, 0, H)
    out = torch.empty((plan.frames(1), T, BINS, 2), device="cuda")
    done, none = 0, 0
    for k, b in enumerate(st.blocks(x, B)):
        out.fill_(7.0)
        r = plan.process(dev(b), out=out)
        f = r.shape[0]
        assert f == calls[k] and same_bits(host(r), rows[done:done + f]) and (host(out)[f:] == 7.0).all(), k
        done, none = done + f, none + (f == 0)
    assert none == sum(1 for c in calls if c == 0) and (none > len(calls) // 2) == (2 * B < H)
    plan.close()


def test_one_call_of_one_sample_and_a_batch_longer_than_the_history(gab):
    T = 3
    x = stream(T)
    one = gab.SpectrumPlan(T, 1, 32, "power")
    r = one.process(dev(x[:, :1].copy()))
    assert r.shape[0] == 0
    hist_is_the_streams_tail(one, x, 1, 32)
    one.close()
    plan = gab.SpectrumPlan(T, 512, 512, "power")
    plan.process(dev(st.blocks(x[:, :512], 512)[0]))
    r = plan.process_batch(dev(st.blocks(x[:, 512:2048], 512)))          # 1536 samples: more than the history holds
    assert r.shape[0] == 3
    hist_is_the_streams_tail(plan, x, 2048, 512)
    r2 = plan.process_batch(dev(st.blocks(x[:, 2048:4096], 512)))
    plan.close()
    ref = gab.SpectrumPlan(T, 512, 512, "power")
    want, _ = run(ref, x)
    ref.close()
    assert same_bits(host(r), want[1:4]) and same_bits(host(r2), want[4:])


def test_after_reset_the_plan_is_a_new_plan(gab):
    T, B, H = 9, 100, 96
    x = stream(T)
    w2 = (st.window_hann() ** 2).astype(np.float32)
    plan = gab.SpectrumPlan(T, B, H, "power", 8)
    plan.set_window(dev(w2))
    plan.set_bands([0, 2, 4, 8, 16, 32, 64, 128, 513])
    first, _ = run(plan, x[:, :2000])
    run(plan, x[:, 2000:2700])                            # leaves a phase and a history behind
    plan.reset()
    hist_is_the_streams_tail(plan, x, 0, H)
    again, _ = run(plan, x[:, :2000])
    plan.close()
    assert same_bits(first, again)                         # the window and the edges stayed
    fresh = gab.SpectrumPlan(T, B, H, "power", 8)
    other, _ = run(fresh, x[:, :2000])
    fresh.close()
    assert not same_bits(first, other)


def test_set_window_mid_stream_keeps_the_history(gab):
    T, B, H = 3, 512, 256
    x = stream(T)
    w2 = np.sqrt(st.window_hann()).astype(np.float32)
    a = gab.SpectrumPlan(T, B, H, "complex")
    head, _ = run(a, x[:, :2048])
    a.set_window(dev(w2))
    hist_is_the_streams_tail(a, x, 2048, H)
    assert same_bits(host(a.state()[1]), w2)
    tail, _ = run(a, x[:, 2048:])
    a.close()
    b = gab.SpectrumPlan(T, B, H, "complex")
    b.set_window(dev(w2))
    allw2, _ = run(b, x)
    b.close()
    c = gab.SpectrumPlan(T, B, H, "complex")
    hann, _ = run(c, x)
    c.close()
    assert same_bits(head, hann[:8]) and same_bits(tail, allw2[8:])        # frame 9 reaches 768 samples back


# ---- isolation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [9, 17])
def test_a_silent_pair_gives_zeros_and_a_pair_depends_on_nothing_outside_itself(gab, T):
    x = stream(T).copy()
    silent = [2, 3, T - 1] + ([10, 11] if T > 11 else [])
    x[silent] = 0.0
    for mode, bands in (("complex", 0), ("power", 0), ("power", 5)):
        plan = gab.SpectrumPlan(T, 512, 256, mode, bands)
        base, _ = run(plan, x, batch=4)
        assert not base[:, silent].any()
        assert base[:, 0].any() and base[:, 4].any()
        loud = (np.random.default_rng(7).standard_normal(x.shape) * 2.0 ** 10).astype(np.float32)
        for q in range((T + 1) // 2):
            own = [t for t in (2 * q, 2 * q + 1) if t < T]
            v = loud.copy()
            v[own] = x[own]
            plan.reset()
            got, _ = run(plan, v, batch=4)
            assert same_bits(got[:, own], base[:, own]), (mode, q)
        plan.close()


@pytest.mark.parametrize("T", [9, 17])
def test_a_pair_aligned_shard_as_its_own_plan_gives_those_tracks_bits(gab, T):
    x = stream(T)
    for mode, bands in (("complex", 0), ("power", 31)):
        whole = gab.SpectrumPlan(T, 100, 96, mode, bands)
        want, _ = run(whole, x)
        whole.close()
        for lo, hi in ((0, 2), (2, 8), (6, T)):
            shard = gab.SpectrumPlan(hi - lo, 100, 96, mode, bands)
            got, _ = run(shard, np.ascontiguousarray(x[lo:hi]))
            shard.close()
            assert same_bits(got, want[:, lo:hi]), (mode, lo, hi)


@pytest.mark.parametrize("H", [256, 96, 1000])
def test_a_nan_stays_in_its_pair_and_in_the_frames_that_hold_it(gab, H):
    T, B = 9, 512
    x = stream(T)
    plan = gab.SpectrumPlan(T, B, H, "power")
    base, _ = run(plan, x)
    ends = np.array(st.frame_ends(0, TOTAL, H))
    for t, a, v in ((0, 1500, np.nan), (T - 1, 1023, np.inf), (3, 2048, -np.inf)):
        d = x.copy()
        d[t, a] = v
        plan.reset()
        got, _ = run(plan, d, batch=2)
        holds = (ends - N <= a) & (a < ends)
        assert 1 <= holds.sum() <= -(-N // H)
        pair = [u for u in (t & ~1, (t & ~1) + 1) if u < T]
        for f in range(len(ends)):
            for u in range(T):
                if u in pair and holds[f]:
                    assert not np.isfinite(got[f, u]).all(), (f, u)
                else:
                    assert same_bits(got[f, u], base[f, u]), (f, u)
    plan.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_each_with_its_text(gab):
    import torch
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()

    def refused(rc, text):
        assert rc == bad and text in lib.gab_last_error().decode(), (rc, lib.gab_last_error())

    for hop in (31, 1025, 0, -5):
        refused(lib.gab_spec_create(ctypes.byref(h), 4, 512, hop, 1, 0), "hop must be 32..1024")
        assert not h.value
    refused(lib.gab_spec_create(ctypes.byref(h), 4, 512, 512, 0, 8), "bands need GAB_SPEC_POWER")
    refused(lib.gab_spec_create(ctypes.byref(h), 4, 512, 512, 1, 65), "bands must be 0..64")
    refused(lib.gab_spec_create(ctypes.byref(h), 4, 512, 512, 2, 0), "mode must be")
    refused(lib.gab_spec_create(ctypes.byref(h), 0, 512, 512, 1, 0), "tracks and bufsize must be > 0")
    refused(lib.gab_spec_create(None, 4, 512, 512, 1, 0), "null plan pointer")
    assert not h.value

    T, B = 3, 512
    x = stream(T)
    plan = gab.SpectrumPlan(T, B, 512, "power", 4)
    first = host(plan.process(dev(st.blocks(x[:, :B], B)[0])))
    with pytest.raises(gab.GabError, match=r"edge 2 \(10\) breaks 0 <= e_0 < e_1"):
        plan.set_bands([0, 10, 10, 20, 30])
    with pytest.raises(gab.GabError, match=r"edge 4 \(514\) breaks"):
        plan.set_bands([0, 1, 2, 3, 514])
    with pytest.raises(gab.GabError, match=r"edge 0 \(-1\) breaks"):
        plan.set_bands([-1, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="bands \\+ 1 = 5"):
        plan.set_bands([0, 1, 2])
    w = st.window_hann()
    for n, v in ((700, np.nan), (0, np.inf), (1023, -np.inf)):
        s = w.copy()
        s[n] = v
        s[min(n + 1, 1023)] = v                           # the first is named
        with pytest.raises(gab.GabError, match="window value %d is not finite; the plan keeps its window" % n):
            plan.set_window(dev(s))
    for s in (np.zeros(N, np.float32), np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(np.float32)):
        with pytest.raises(gab.GabError, match="the window's sum is zero; the plan keeps its window"):
            plan.set_window(dev(s))
    n = ctypes.c_int(0)
    t = torch.zeros(T * B, device="cuda")
    ptr = ctypes.c_void_p(t.data_ptr())
    refused(lib.gab_spec_process(plan._h, None, ptr, ctypes.byref(n), None), "gab_spec_process: null pointer")
    refused(lib.gab_spec_process(plan._h, ptr, None, ctypes.byref(n), None), "gab_spec_process: null pointer")
    refused(lib.gab_spec_process(plan._h, ptr, ptr, None, None), "gab_spec_process: null pointer")
    refused(lib.gab_spec_process(None, ptr, ptr, ctypes.byref(n), None), "gab_spec_process: null pointer")
    refused(lib.gab_spec_process_batch(plan._h, ptr, ptr, 0, ctypes.byref(n), None), "n_buffers must be > 0")
    refused(lib.gab_spec_set_window(plan._h, None, None), "gab_spec_set_window: null pointer")
    refused(lib.gab_spec_set_bands(plan._h, None), "gab_spec_set_bands: null pointer")
    refused(lib.gab_spec_frames(plan._h, 1, None), "gab_spec_frames: null pointer")
    refused(lib.gab_spec_state(plan._h, None, None, None), "gab_spec_state: null pointer")
    refused(lib.gab_spec_reset(None, None), "gab_spec_reset: null pointer")
    refused(lib.gab_spec_destroy(None), "gab_spec_destroy: null pointer")
    # every refusal left the plan as it was: the window, the edges, the history and the position
    assert same_bits(host(plan.state()[1]), w)
    hist_is_the_streams_tail(plan, x, B, 512)
    plan.reset()
    assert same_bits(host(plan.process(dev(st.blocks(x[:, :B], B)[0]))), first)
    plan.close()
    nobands = gab.SpectrumPlan(T, B, 512, "power")
    refused(lib.gab_spec_set_bands(nobands._h, (ctypes.c_int * 2)(0, 513)), "the plan has no bands")
    nobands.close()
    odd = gab.SpectrumPlan(T, 100, 96, "power")
    with pytest.raises(ValueError, match="hop 96 does not divide bufsize 100"):
        odd.prepare(torch.zeros(T * 100, device="cuda"), torch.zeros(2 * T * BINS, device="cuda"))
    odd.close()


# ---- capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,bands,H", [("complex", 0, 256), ("power", 31, 512)])
def test_a_captured_process_replays_to_the_bits_of_plain_calls(gab, mode, bands, H):
    import torch
    T, B = 9, 512
    x = stream(T)
    bl = st.blocks(x, B)
    ref = gab.SpectrumPlan(T, B, H, mode, bands)
    want, _ = run(ref, x)
    ref.close()
    per = B // H
    plan = gab.SpectrumPlan(T, B, H, mode, bands)
    assert same_bits(host(plan.process(dev(bl[0]))), want[:per])          # buffer 0 by a plain call
    xin = torch.zeros(T * B, device="cuda")
    out = torch.zeros((per, T) + plan.row_shape, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(xin, out)
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    hist_is_the_streams_tail(plan, x, B, H)                # the capture recorded the launches without running them
    for k in range(1, 5):
        xin.copy_(dev(bl[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(host(out), want[k * per:(k + 1) * per]), k
        hist_is_the_streams_tail(plan, x, (k + 1) * B, H)
    del graph
    plan.close()
