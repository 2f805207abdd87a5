"""The resynthesis plan (gab_resyn_*, ResynthesisPlan) on the device, against resynthesis_twin.py.

The transform is held by a bound, per track and frame: max_n |u - u64| / (peak_t + peak_p) <= FACTOR c_twin, c_twin the
twin's figure on the same rows.  The device's own u_j come out of a plan at H = B = 1024 under an all-ones window: a call's
output is the previous frame's u, bit for bit (0 + u).  Everything around the transform is exact: with those u_j the
twin's Adder gives the device's outputs and its accumulator after every call, however the stream is cut, batched or
aligned, across a reset and a set_window.  Track counts 1, 2, 3, 9, 17: an odd last track, more than one workgroup, a
partly empty workgroup.  Streams of a few thousand samples."""
import ctypes

import numpy as np
import pytest

import conv_pair_twin as tw
import resynthesis_twin as rt
import spectrum_twin as st
from test_conv_plan_state_gpu import dev, gab, host, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

TRACKS = [1, 2, 3, 9, 17]
N, BINS = rt.N, rt.BINS
F32 = np.float32
# The project's own factor for this transform (test_spectrum_gpu.FACTOR, test_fft_levels_gpu.held).  Measured on these
# rows: 2.28 to 3.75 (profiles/r26_resynthesis.txt); the round trip 2.0 to 3.5 times the twin chain's own error.
FACTOR = 4.0
# (H, B): every class of H | B, H does not divide B, B < H, B > N
CENSUS = [(32, 64), (32, 100), (100, 100), (100, 64), (100, 1536), (256, 1), (256, 512), (256, 1536), (512, 100),
          (512, 512), (512, 1536), (1024, 64), (1024, 512), (1024, 1536)]
CLASSES = {"H | B": lambda H, B: B % H == 0, "H does not divide B": lambda H, B: B % H != 0,
           "B < H": lambda H, B: B < H, "B > N": lambda H, B: B > N}

_pool = {}


def up(a):
    """A (writable) copy of a on the device: the pools are read-only."""
    return dev(np.array(a, F32))


def window_for(H):
    return rt.dual_window(st.window_hann(), H)


def device_frames(gab, rows):
    """u [F, T, 1024] of rows [F, T, 513, 2] as the device transforms them: a plan at H = B = 1024 under all ones, one
    frame a buffer, whose output block k + 1 is frame k's u (0 + u)."""
    F, T = rows.shape[:2]
    plan = gab.ResynthesisPlan(T, 1024, 1024)
    plan.set_window(dev(np.ones(N, F32)))
    fed = np.concatenate([rows, np.zeros((1, T, BINS, 2), F32)])
    out = host(plan.process_batch(dev(fed), F + 1))
    plan.close()
    assert out.shape == (F + 1, T, N) and not out[0].any()
    return out[1:].copy()


def pool(gab, T, F=100):
    """(rows [F, T, 513, 2], the device's u [F, T, 1024]) of track count T, made once and never changed."""
    if (T, F) not in _pool:
        rows = rt.noise_rows(F, T, seed=300 + T)
        u = device_frames(gab, rows)
        rows.setflags(write=False)
        u.setflags(write=False)
        _pool[T, F] = (rows, u)
    return _pool[T, F]


def off_by_4_bytes(n):
    import torch
    t = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[1:]
    assert v.data_ptr() % 16 == 4
    return v


def sizes_for(nb, pattern):
    sizes, left = [], nb
    while left:
        for m in pattern:
            if left == 0:
                break
            sizes.append(min(m, left))
            left -= sizes[-1]
    return sizes


def drive(plan, twin, rows, u, sizes, first=0, single=True, off=False):
    """Frames first.. of the pool through `plan` and its twin in calls of sizes[i] buffers; the outputs and the
    accumulator must agree bit for bit after every call.  Returns the next unused frame."""
    T, B, f = plan.tracks, plan.bufsize, first
    for i, n in enumerate(sizes):
        k = plan.count(n)
        assert k == twin.count(n) and k <= plan.frames(n) == rt.capacity(B, plan.hop, n)
        r = up(rows[f:f + k])
        out = off_by_4_bytes(n * T * B) if off else None
        got = plan.process(r, out=out) if (single and n == 1) else plan.process_batch(r, n, out=out)
        want = twin.take(u[f:f + k], n)
        assert same_bits(host(got).reshape(want.shape), want), (i, n, k)
        acc, _, phase = plan.state()
        assert same_bits(host(acc), twin.acc) and phase == twin.p % plan.hop, (i, n, k)
        f += k
    return f


# ---- the transform ---------------------------------------------------------------------------------------------------
def test_the_census_names_every_class():
    for name, member in CLASSES.items():
        assert any(member(H, B) for H, B in CENSUS), name
    assert {H for H, _ in CENSUS} == {32, 100, 256, 512, 1024} and {B for _, B in CENSUS} == {1, 64, 100, 512, 1536}


@pytest.mark.parametrize("T", TRACKS)
def test_every_track_and_frame_is_within_4_c_twin_of_its_pairs_peak(gab, T):
    rows = rt.noise_rows(4, T, seed=200 + T)               # track t at conv_pair_twin.levels(T): unequal within a pair
    u64 = rt.truth(rows)
    c, level = rt.figures(rt.frames_f32(rows), u64)
    c_twin = tw.c_max(c)
    u = device_frames(gab, rows)
    cg, _ = rt.figures(u, u64)
    print("\nresynthesis T %d c_twin %.3g c_gpu %.3g ratio %.2f" % (T, c_twin, tw.c_max(cg), tw.c_max(cg) / c_twin))
    assert 0 < c_twin <= 1e-6 and (level > 0).all()
    assert (cg <= FACTOR * c_twin).all(), cg.max() / c_twin
    # a frame a call gives the same bits as the frames of one batch, and the accumulator is the frame itself
    plan = gab.ResynthesisPlan(T, 1024, 1024)
    plan.set_window(dev(np.ones(N, F32)))
    for f in range(4):
        out = host(plan.process(up(rows[f:f + 1])))
        assert same_bits(host(plan.state()[0]), u[f]) and (same_bits(out, u[f - 1]) if f else not out.any())
    plan.close()


@pytest.mark.parametrize("T", [9, 17])
def test_a_silent_pair_gives_zeros_and_a_pair_depends_on_nothing_outside_itself(gab, T):
    rows = rt.noise_rows(3, T, seed=210 + T).copy()
    silent = [2, 3, T - 1] + ([10, 11] if T > 11 else [])
    rows[:, silent] = 0.0
    base = device_frames(gab, rows)
    assert not base[:, silent].any() and base[:, 0].any() and base[:, 4].any()
    loud = (np.random.default_rng(7).standard_normal(rows.shape) * 2.0 ** 10).astype(F32)
    for q in range((T + 1) // 2):
        own = [t for t in (2 * q, 2 * q + 1) if t < T]
        v = loud.copy()
        v[:, own] = rows[:, own]
        assert same_bits(device_frames(gab, v)[:, own], base[:, own]), q


@pytest.mark.parametrize("T", [3, 9])
def test_garbage_in_the_imaginary_parts_of_bins_0_and_512_gives_the_bits_of_zeros(gab, T):
    rows = rt.noise_rows(3, T, seed=220 + T).copy()
    clean = rows.copy()
    clean[..., 0, 1] = 0.0
    clean[..., 512, 1] = 0.0
    base = device_frames(gab, clean)
    assert same_bits(device_frames(gab, rows), base)
    rows[0, :, 0, 1], rows[1, :, 512, 1], rows[2, 0, 0, 1] = np.nan, np.inf, -2.0 ** 100
    assert same_bits(device_frames(gab, rows), base)


# ---- the overlap-add, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", CENSUS)
def test_outputs_and_accumulator_are_the_twins_however_the_stream_is_cut(gab, H, B):
    T = 3
    rows, u = pool(gab, T, 200)
    nb = 600 if B == 1 else max(4, -(-2600 // B))
    assert rt.count(0, nb * B, H) <= 200
    g = window_for(H)
    plan = gab.ResynthesisPlan(T, B, H)
    assert same_bits(host(plan.state()[1]), g) and plan.latency == N
    twin = rt.Adder(T, B, H, g)
    drive(plan, twin, rows, u, [1] * nb)                                  # per buffer
    for pattern, single, off in (((1, 3, 2, 5), False, False), ((nb,), False, False), ((2, 1, 4), True, True)):
        if B == 1 and len(pattern) > 1:
            pattern = tuple(37 * m for m in pattern)
        plan.reset()
        twin.reset()
        drive(plan, twin, rows, u, sizes_for(nb, pattern), single=single, off=off)
    plan.close()


@pytest.mark.parametrize("T", TRACKS)
def test_every_track_count_per_buffer_and_batched(gab, T):
    H, B, nb = 100, 512, 5
    rows, u = pool(gab, T, 30)
    plan, twin = gab.ResynthesisPlan(T, B, H), rt.Adder(T, B, H, window_for(H))
    drive(plan, twin, rows, u, [1] * nb)
    plan.reset()
    twin.reset()
    drive(plan, twin, rows, u, [2, 3], off=True)
    plan.close()


@pytest.mark.parametrize("H,B", [(256, 512), (100, 64)])
def test_a_reset_and_a_set_window_mid_stream(gab, H, B):
    T = 3
    rows, u = pool(gab, T, 200)
    g, g2 = window_for(H), (window_for(H) * np.linspace(0.5, 2.0, N)).astype(F32)
    plan, twin = gab.ResynthesisPlan(T, B, H), rt.Adder(T, B, H, g)
    k = 2048 // B
    f = drive(plan, twin, rows, u, [1] * k)
    before = host(plan.state()[0])
    plan.set_window(dev(g2))
    twin.set_window(g2)
    acc, w, phase = plan.state()
    assert same_bits(host(w), g2) and same_bits(host(acc), before) and phase == twin.p % H   # the accumulator stays
    f = drive(plan, twin, rows, u, sizes_for(k, (1, 3)), first=f)
    plan.reset()
    twin.reset()
    acc, w, phase = plan.state()
    assert not host(acc).any() and phase == 0 and same_bits(host(w), g2)      # the window stays
    drive(plan, twin, rows, u, sizes_for(k, (2, 1)), first=f)
    plan.close()


@pytest.mark.parametrize("H,B,seed", [(100, 64, 1), (256, 512, 2), (1000, 100, 3)])
def test_a_seeded_walk_of_process_batch_reset_and_set_window(gab, H, B, seed):
    T = 9
    rows, u = pool(gab, T, 100)
    rng = np.random.default_rng(seed)
    g = window_for(min(H, 512))
    plan, twin = gab.ResynthesisPlan(T, B, H), rt.Adder(T, B, H, window_for(H))
    f = 0
    for step in range(40):
        what = rng.choice(["process", "batch", "batch", "reset", "window"], p=[0.4, 0.2, 0.2, 0.1, 0.1])
        if what == "reset":
            plan.reset()
            twin.reset()
        elif what == "window":
            w = (g * F32(rng.uniform(0.25, 4.0))).astype(F32)
            plan.set_window(dev(w))
            twin.set_window(w)
        else:
            n = 1 if what == "process" else int(rng.integers(1, 5))
            if f + rt.capacity(B, H, n) > len(rows):
                f = 0                                       # any rows may follow any: the plan does not know
            f = drive(plan, twin, rows, u, [n], first=f, single=what == "process", off=bool(rng.integers(2)))
    plan.close()


def test_a_call_of_one_sample_and_a_call_without_a_frame_leave_the_rows_alone_and_shift(gab):
    import torch
    T, H = 3, 32
    rows, u = pool(gab, T, 30)
    one, twin = gab.ResynthesisPlan(T, 1, H), rt.Adder(T, 1, H, window_for(H))
    f = drive(one, twin, rows, u, [1] * 70)                # 70 calls of one sample: two take a frame
    assert f == 2
    filled = torch.full((T * BINS * 2,), 7.0, device="cuda")
    out, n = torch.zeros(T, device="cuda"), ctypes.c_int(-1)
    before = host(one.state()[0])
    assert one.count(1) == 0
    rc = gab.lib.gab_resyn_process(one._h, ctypes.c_void_p(filled.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                   ctypes.byref(n), None)
    torch.cuda.synchronize()
    assert rc == 0 and n.value == 0 and (host(filled) == 7.0).all()
    after = host(one.state()[0])
    assert same_bits(host(out), before[:, 0]) and same_bits(after[:, :N - 1], before[:, 1:]) and not after[:, N - 1].any()
    one.close()
    plan = gab.ResynthesisPlan(T, 100, 512)                # a call that takes a frame never writes its rows either
    r = up(rows[:1])
    plan.process_batch(up(rows[:0]), 5)
    assert plan.count(1) == 1
    plan.process(r)
    assert same_bits(host(r), rows[:1])
    with pytest.raises(ValueError, match="takes exactly 0 frames"):
        plan.process(r)
    plan.close()


# ---- the round trip --------------------------------------------------------------------------------------------------
def pair_err(y, ref):
    """max |y - ref| per pair of tracks: a track's absolute error follows its pair's."""
    e = np.abs(np.asarray(y, np.float64) - ref).max(axis=1)
    e = np.concatenate([e, np.zeros(len(e) % 2)])
    return e.reshape(-1, 2).max(axis=1)


def masked64(x, H, mask):
    """The float64 chain with `mask` [513] on every row: windowed float32 frames, rfft, mask, irfft, the float32 dual
    window's values, overlap-add, all in float64.  [T, total]."""
    total = x.shape[1]
    ends = rt.frame_ends(0, total, H)
    X = st.truth(st.windowed(x, ends, st.window_hann())) * mask[None, None, :]
    v = np.fft.irfft(X, n=N, axis=-1) * window_for(H).astype(np.float64)[None, None, :]
    y = np.zeros((x.shape[0], total + N))
    for vj, e in zip(v, ends):
        y[:, e:e + N] += vj
    return y[:, :total]


@pytest.mark.parametrize("H,B", [(256, 512), (512, 512), (100, 512)])
@pytest.mark.parametrize("masked", [False, True])
def test_analyser_to_resynthesis_returns_the_stream_delayed_by_1024(gab, H, B, masked):
    """The bound is four times the error of the twin chain (analyser twin -> resynthesis twin in float32) on the same
    stream, per pair: against the delayed input, or under a mask against the float64 chain with the same mask."""
    import torch
    T, total = 3, 4096
    x = st.noise(T, total, seed=400 + H)
    mask = np.ones(BINS, F32)
    if masked:
        mask[100:] = 0.0
        mask[:100] = np.linspace(1.0, 0.25, 100).astype(F32)
    ref = masked64(x, H, mask.astype(np.float64)) if masked else np.concatenate([np.zeros((T, N)), x[:, :total - N]], 1)
    rows_twin = (rt.analyse(x, H) * mask[None, None, :, None]).astype(F32)
    y_twin, _ = rt.overlap_add(rt.frames_f32(rows_twin), rt.frame_ends(0, total, H), window_for(H), total)
    e_twin = pair_err(y_twin, ref)
    spec, resyn = gab.SpectrumPlan(T, B, H, "complex"), gab.ResynthesisPlan(T, B, H)
    m = dev(mask)[None, None, :, None]
    out = []
    for b in st.blocks(x, B):
        rows = spec.process(dev(b))
        out.append(host(resyn.process((rows * m).contiguous() if masked else rows)))
    spec.close()
    resyn.close()
    y = np.concatenate(out, axis=1)
    e_gpu = pair_err(y, ref)
    print("\nresynthesis round trip H %d masked %d e_twin %s e_gpu %s ratio %.2f"
          % (H, masked, e_twin, e_gpu, (e_gpu / e_twin).max()))
    assert (e_twin > 0).all() and (e_twin <= 4e-6).all()
    assert (e_gpu <= 4.0 * e_twin).all(), e_gpu / e_twin
    assert not y[:, :H].any()


# ---- capture ---------------------------------------------------------------------------------------------------------
def test_both_plans_captured_in_one_graph_replay_to_the_bits_of_plain_calls(gab):
    import torch
    T, B, H = 9, 512, 256
    x = st.noise(T, 4096, seed=77)
    bl = st.blocks(x, B)
    spec, resyn = gab.SpectrumPlan(T, B, H, "complex"), gab.ResynthesisPlan(T, B, H)
    want = [host(resyn.process(spec.process(dev(b)))) for b in bl]
    spec.reset()
    resyn.reset()
    assert same_bits(host(resyn.process(spec.process(dev(bl[0])))), want[0])      # buffer 0 by plain calls
    xin = torch.zeros(T * B, device="cuda")
    rows = torch.zeros((B // H, T, BINS, 2), device="cuda")
    out = torch.zeros((T, B), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        a, b = spec.prepare(xin, rows), resyn.prepare(rows, out)
        with torch.cuda.graph(graph, stream=side):
            spec.launch(a)
            resyn.launch(b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in range(1, 6):
        xin.copy_(dev(bl[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(host(out), want[k]), k
    del graph
    spec.close()
    resyn.close()
    odd = gab.ResynthesisPlan(T, 100, 96)
    with pytest.raises(ValueError, match="ResynthesisPlan.prepare: hop 96 does not divide bufsize 100"):
        odd.prepare(torch.zeros(T * BINS * 2, device="cuda"), torch.zeros(T * 100, device="cuda"))
    odd.close()


# ---- isolation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(256, 512), (100, 64), (1000, 512)])
def test_a_nan_stays_in_its_pair_and_in_its_frames_1024_samples(gab, H, B):
    T, nb = 9, 4096 // B
    rows, _ = pool(gab, T, 100)
    ends = rt.frame_ends(0, nb * B, H)

    def run(r):
        plan = gab.ResynthesisPlan(T, B, H)
        y = host(plan.process_batch(up(r[:len(ends)]), nb)).transpose(1, 0, 2).reshape(T, nb * B)
        acc = host(plan.state()[0])
        plan.close()
        return np.concatenate([y, acc], axis=1)            # output sample o, and the accumulator behind the stream

    base = run(rows)
    assert np.isfinite(base).all()
    for f, t, k, v in ((1, 0, 17, np.nan), (len(ends) // 2, T - 1, 0, np.inf), (len(ends) - 1, 3, 511, -np.inf)):
        r = rows.copy()
        r[f, t, k, 0] = v
        got = run(r)
        struck = np.zeros(got.shape[1], bool)
        struck[ends[f]:ends[f] + N] = True                 # frame j's samples y[jH - N .. jH) are outputs jH .. jH + N
        pair = [s for s in (t & ~1, (t & ~1) + 1) if s < T]
        for s in range(T):
            if s in pair:
                assert not np.isfinite(got[s, struck]).any() and same_bits(got[s, ~struck], base[s, ~struck]), (f, s)
            else:
                assert same_bits(got[s], base[s]), (f, s)


@pytest.mark.parametrize("T", [9, 17])
def test_a_pair_aligned_shard_as_its_own_plan_gives_those_tracks_bits(gab, T):
    H, B, nb = 100, 100, 12
    rows, _ = pool(gab, T, 30)
    k = rt.count(0, nb * B, H)
    whole = gab.ResynthesisPlan(T, B, H)
    want = host(whole.process_batch(up(rows[:k]), nb))
    wacc = host(whole.state()[0])
    whole.close()
    for lo, hi in ((0, 2), (2, 8), (6, T)):
        shard = gab.ResynthesisPlan(hi - lo, B, H)
        got = host(shard.process_batch(up(rows[:k, lo:hi]), nb))
        assert same_bits(got, want[:, lo:hi]) and same_bits(host(shard.state()[0]), wacc[lo:hi]), (lo, hi)
        shard.close()


# ---- refusals and state ----------------------------------------------------------------------------------------------
def test_refusals_each_with_its_text(gab):
    import torch
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()

    def refused(rc, text):
        assert rc == bad and text in lib.gab_last_error().decode(), (rc, lib.gab_last_error())

    for hop in (31, 1025, 0, -5):
        refused(lib.gab_resyn_create(ctypes.byref(h), 4, 512, hop), "gab_resyn_create: hop must be 32..1024")
        assert not h.value
    refused(lib.gab_resyn_create(ctypes.byref(h), 0, 512, 512), "tracks and bufsize must be > 0")
    refused(lib.gab_resyn_create(ctypes.byref(h), 4, 0, 512), "tracks and bufsize must be > 0")
    refused(lib.gab_resyn_create(ctypes.byref(h), (1 << 26) + 1, 512, 512), "more than 2^23 workgroups")
    refused(lib.gab_resyn_create(None, 4, 512, 512), "null plan pointer")
    assert not h.value

    T, B, H = 3, 512, 512
    rows, u = pool(gab, T, 30)
    plan, twin = gab.ResynthesisPlan(T, B, H), rt.Adder(T, B, H, window_for(H))
    f = drive(plan, twin, rows, u, [1, 1])
    g = window_for(H)
    for n, v in ((700, np.nan), (0, np.inf), (1023, -np.inf)):
        s = g.copy()
        s[n] = v
        s[min(n + 1, 1023)] = v                           # the first is named
        with pytest.raises(gab.GabError, match="window value %d is not finite; the plan keeps its window" % n):
            plan.set_window(dev(s))
    n = ctypes.c_int(0)
    t = torch.zeros(T * BINS * 2, device="cuda")
    o = torch.zeros(T * B + 2, device="cuda")
    ptr, optr = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(o.data_ptr())
    for args in ((plan._h, None, optr, ctypes.byref(n)), (plan._h, ptr, None, ctypes.byref(n)),
                 (plan._h, ptr, optr, None), (None, ptr, optr, ctypes.byref(n))):
        refused(lib.gab_resyn_process(*args, None), "gab_resyn_process: null pointer")
    refused(lib.gab_resyn_process_batch(plan._h, ptr, optr, 0, ctypes.byref(n), None), "n_buffers must be > 0")
    refused(lib.gab_resyn_process_batch(plan._h, ptr, optr, (1 << 22) - 1, ctypes.byref(n), None),
            "n_buffers * bufsize must be below 2^31 - 1024")
    refused(lib.gab_resyn_process(plan._h, ctypes.c_void_p(t.data_ptr() + 4), optr, ctypes.byref(n), None),
            "d_rows must lie on an 8-byte boundary")
    refused(lib.gab_resyn_process(plan._h, ptr, ctypes.c_void_p(t.data_ptr() + 8), ctypes.byref(n), None),
            "d_rows and d_out overlap")
    refused(lib.gab_resyn_set_window(plan._h, None, None), "gab_resyn_set_window: null pointer")
    refused(lib.gab_resyn_frames(plan._h, 1, None), "gab_resyn_frames: null pointer")
    refused(lib.gab_resyn_frames(plan._h, 0, ctypes.byref(n)), "n_buffers must be > 0")
    refused(lib.gab_resyn_count(plan._h, 1, None), "gab_resyn_count: null pointer")
    refused(lib.gab_resyn_count(plan._h, -1, ctypes.byref(n)), "n_buffers must be > 0")
    refused(lib.gab_resyn_state(plan._h, None, None, None), "gab_resyn_state: null pointer")
    refused(lib.gab_resyn_latency(plan._h, None), "gab_resyn_latency: null pointer")
    refused(lib.gab_resyn_reset(None, None), "gab_resyn_reset: null pointer")
    refused(lib.gab_resyn_destroy(None), "gab_resyn_destroy: null pointer")
    with pytest.raises(ValueError, match="takes exactly 1 frames"):
        plan.process(up(rows[:2]))
    # every refusal left the plan as it was: the window, the accumulator and the position
    acc, w, phase = plan.state()
    assert same_bits(host(w), g) and same_bits(host(acc), twin.acc) and phase == twin.p % H
    drive(plan, twin, rows, u, [1, 2], first=f)
    plan.close()


@pytest.mark.parametrize("H,B", [(100, 64), (512, 512), (1024, 1536)])
def test_state_after_reset_and_the_first_outputs(gab, H, B):
    T = 3
    rows, u = pool(gab, T, 200)
    plan = gab.ResynthesisPlan(T, B, H)
    g = host(plan.state()[1])
    assert same_bits(g, window_for(H)) and plan.latency == N == rt.LATENCY
    assert same_bits(g, host(gab.synthesis_window(dev(st.window_hann()), H)))
    nb = -(-2048 // B)
    k = plan.count(nb)
    first = host(plan.process_batch(up(rows[:k]), nb))
    plan.process_batch(up(rows[:plan.count(3)]), 3)       # leaves a phase and an accumulator behind
    plan.reset()
    acc, w, phase = plan.state()
    assert not host(acc).any() and not host(acc).view(np.uint32).any() and phase == 0 and same_bits(host(w), g)
    assert plan.count(nb) == k
    again = host(plan.process_batch(up(rows[:k]), nb))
    plan.close()
    assert same_bits(first, again)
    y = again.transpose(1, 0, 2).reshape(T, nb * B)
    # +0.0f, then y at negative indices as summed
    assert not np.ascontiguousarray(y[:, :H]).view(np.uint32).any() and (H == N or y[:, H:N].any())
