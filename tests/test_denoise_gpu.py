"""The denoise plan (gab_dn_*, DenoisePlan) on the device.

The contract is a composition: the fused form equals SpectrumPlan(complex) -> DenoisePlan.process_rows -> ResynthesisPlan
bit for bit (outputs, history, accumulator, mask, phase), after every call of any cut.  The rows form is held bit for bit
to denoise_twin.Gate on the device's own bins, so the gate's arithmetic is the header's; P's bits are held to
SpectrumPlan(mode="power") without knowing them in advance; and the whole chain is held to the float64 truth by the
project's factor for this transform where no decision can flip.  Track counts 1, 2, 3, 9, 17: a lone last track, more
than one workgroup, an odd pair count.  Streams of 4096 to 8192 samples."""
import ctypes

import numpy as np
import pytest

import denoise_twin as dt
import resynthesis_twin as rt
import spectrum_twin as st
from test_conv_plan_state_gpu import dev, gab, host, same_bits  # noqa: F401
from test_resynthesis_gpu import CENSUS, off_by_4_bytes, sizes_for

pytestmark = pytest.mark.gpu

TRACKS = [1, 2, 3, 9, 17]
N, BINS = dt.N, dt.BINS
F32 = np.float32
FACTOR = 4.0          # the project's factor for this transform (test_resynthesis_gpu.FACTOR)
LEVEL = 0.002         # the mean power of a bin of uniform(-1, 1) noise under Hann: (1 / 3) 4 sum w^2 / S^2


def unit_noise(T, total, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (T, total)).astype(F32)


def up(a):
    return dev(np.array(a, F32))


class Composed:
    """What the fused form must equal: three plans of the same T, B and H, the middle one used through its rows form."""

    def __init__(self, gab, T, B, H):
        self.spec, self.gate, self.resyn = gab.SpectrumPlan(T, B, H, "complex"), gab.DenoisePlan(T, B, H), gab.ResynthesisPlan(T, B, H)

    def process(self, xs, n, single):
        if single and n == 1:
            return self.resyn.process(self.gate.process_rows(self.spec.process(xs).contiguous()))
        rows = self.gate.process_rows(self.spec.process_batch(xs).contiguous())
        return self.resyn.process_batch(rows, n)

    def reset(self):
        for p in (self.spec, self.gate, self.resyn):
            p.reset()

    def state(self):
        hist, _, phase = self.spec.state()
        acc, _, phase2 = self.resyn.state()
        assert phase == phase2
        return hist, acc, self.gate.state()[2], phase

    def close(self):
        for p in (self.spec, self.gate, self.resyn):
            p.close()


def set_tables(plans, thr=None, params=None, first=0):
    for p in plans:
        put = (lambda a: a) if isinstance(p, dt.Gate) else up             # the twin takes numpy
        if thr is not None:
            p.set_thresholds(put(thr), first)
        if params is not None:
            p.set_params(put(params), first)


def same_state(fused, comp):
    a, b = fused.state(), comp.state()
    return all(same_bits(host(u), host(v)) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]


def drive(fused, comp, bl, sizes, first=0, single=True, off=False):
    """Buffers first.. of bl [nb, T, B] through the fused plan and the composition in calls of sizes[i] buffers: outputs
    and the four states agree bit for bit after every call.  Returns (the next buffer, the fused outputs [T, samples])."""
    T, B, k, outs = fused.tracks, fused.bufsize, first, []
    for i, n in enumerate(sizes):
        xs = dev(bl[k:k + n])
        if off:
            xin, out = off_by_4_bytes(n * T * B), off_by_4_bytes(n * T * B)
            xin.copy_(xs.ravel())
        else:
            xin, out = xs, None
        got = fused.process(xin, out=out) if (single and n == 1) else fused.process_batch(xin, out=out)
        want = comp.process(xs[0] if (single and n == 1) else xs, n, single)
        got, want = host(got).reshape(n, T, B), host(want).reshape(n, T, B)
        assert same_bits(got, want), (i, n, k)
        assert same_state(fused, comp), (i, n, k)
        outs.append(dt.stream_of(got))
        k += n
    return k, np.concatenate(outs, axis=1)


def device_rows(gab, x, H, mode="complex"):
    """The rows of the whole stream x [T, total] as a SpectrumPlan on the device writes them."""
    T, total = x.shape
    plan = gab.SpectrumPlan(T, total, H, mode)
    rows = host(plan.process(dev(x))).copy()
    plan.close()
    return rows


# ---- 1. the rows form against the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TRACKS)
def test_rows_form_is_the_twins_gate_bit_for_bit_in_place_and_apart_across_sets(gab, T):
    H = 256
    rows = device_rows(gab, unit_noise(T, 6144, seed=10 + T), H)          # 24 frames
    thr, params = dt.seeded_tables(T, 20 + T, LEVEL)
    thr2, params2 = dt.seeded_tables(T, 30 + T, LEVEL)
    plan, twin = gab.DenoisePlan(T, 512, H), dt.Gate(T)
    set_tables([plan, twin], thr, params)
    before = [host(s) for s in plan.state()[:2]]
    f = 0
    for i, n in enumerate((7, 0, 1, 7, 1, 0, 7)):
        if i == 3:
            set_tables([plan, twin], thr=thr2[:1], first=T - 1)           # a set of each table mid-stream, over a range
        if i == 4:
            set_tables([plan, twin], params=params2)
        r = up(rows[f:f + n])
        if i % 2:
            got = plan.process_rows(r)                                    # apart: the input stays
            assert same_bits(host(r), rows[f:f + n])
        else:
            got = plan.process_rows(r, out=r)                             # in place
        want = twin.take(rows[f:f + n])
        assert same_bits(host(got).reshape(want.shape), want), (i, n)
        assert same_bits(host(plan.state()[2]), twin.mask), (i, n)
        f += n
    t, p = plan.tables()
    assert same_bits(host(t), twin.thr) and same_bits(host(p), twin.params)
    hist, acc, mask, phase = plan.state()
    assert same_bits(host(hist), before[0]) and same_bits(host(acc), before[1]) and phase == 0    # the mask only
    assert (twin.mask < 1.0).any() and (twin.mask > 0.5).any()
    plan.close()


# ---- 2. fused equals composed ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", CENSUS)
def test_fused_equals_the_composition_however_the_stream_is_cut(gab, H, B):
    T = 3
    nb = 600 if B == 1 else max(4, -(-4096 // B))
    x = unit_noise(T, nb * B, seed=H + B)
    bl = st.blocks(x, B)
    thr, params = dt.seeded_tables(T, H + B, LEVEL)
    fused, comp = gab.DenoisePlan(T, B, H), Composed(gab, T, B, H)
    assert fused.latency == N == dt.LATENCY
    set_tables([fused, comp.gate], thr, params)
    _, first = drive(fused, comp, bl, [1] * nb)                            # per buffer
    assert nb * B < H + N or (host(fused.state()[2]) < 1.0).any()
    for pattern, single, off in (((1, 3, 2, 5), False, False), ((nb,), False, False), ((2, 1, 4), True, True)):
        if B == 1 and len(pattern) > 1:
            pattern = tuple(37 * m for m in pattern)
        fused.reset()                                                      # across a reset: the tables stay
        comp.reset()
        _, y = drive(fused, comp, bl, sizes_for(nb, pattern), single=single, off=off)
        assert same_bits(y, first), pattern                                # the cut does not show
    fused.close()
    comp.close()


@pytest.mark.parametrize("T", TRACKS)
def test_every_track_count_per_buffer_and_batched_and_a_new_plan_is_transparent(gab, T):
    H, B, nb = 100, 512, 8
    bl = st.blocks(unit_noise(T, nb * B, seed=50 + T), B)
    fused, comp = gab.DenoisePlan(T, B, H), Composed(gab, T, B, H)
    # a new plan's tables: the bits of SpectrumPlan -> ResynthesisPlan alone
    spec, resyn = gab.SpectrumPlan(T, B, H, "complex"), gab.ResynthesisPlan(T, B, H)
    _, y = drive(fused, comp, bl, [1, 3])
    plain = [host(resyn.process(spec.process(dev(bl[0])))), host(resyn.process_batch(spec.process_batch(dev(bl[1:4])), 3))]
    assert same_bits(y, np.concatenate([plain[0], dt.stream_of(plain[1])], axis=1))
    assert (host(fused.state()[2]) == 1.0).all()
    spec.close()
    resyn.close()
    thr, params = dt.seeded_tables(T, 60 + T, LEVEL)
    set_tables([fused, comp.gate], thr, params)
    k, _ = drive(fused, comp, bl, [1, 1], first=4)
    drive(fused, comp, bl, [2], first=k, off=True)
    assert (host(fused.state()[2]) < 1.0).any()
    fused.close()
    comp.close()


@pytest.mark.parametrize("H,B,seed", [(100, 64, 1), (256, 512, 2), (1000, 100, 3)])
def test_a_seeded_walk_of_process_batch_sets_and_reset(gab, H, B, seed):
    T = 9
    rng = np.random.default_rng(seed)
    bl = st.blocks(unit_noise(T, 64 * B, seed=70 + seed), B)
    fused, comp = gab.DenoisePlan(T, B, H), Composed(gab, T, B, H)
    k = 0
    for step in range(36):
        what = rng.choice(["process", "batch", "batch", "reset", "thr", "params"], p=[0.35, 0.2, 0.2, 0.05, 0.1, 0.1])
        if what == "reset":
            fused.reset()
            comp.reset()
            assert same_state(fused, comp)
        elif what in ("thr", "params"):
            lo = int(rng.integers(T))
            n = int(rng.integers(1, T - lo + 1))
            thr, params = dt.seeded_tables(T, int(rng.integers(1 << 30)), LEVEL)
            set_tables([fused, comp.gate], thr[:n] if what == "thr" else None, params[:n] if what == "params" else None, lo)
            assert same_state(fused, comp)
        else:
            n = 1 if what == "process" else int(rng.integers(1, 6))
            if k + n > len(bl):
                k = 0                                       # any buffers may follow any: the plan does not know
            k, _ = drive(fused, comp, bl, [n], first=k, single=what == "process", off=bool(rng.integers(2)))
    fused.close()
    comp.close()


# ---- 3. P's bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 9])
def test_the_power_compared_is_the_power_modes_bit_for_bit(gab, T):
    H = 512
    x = unit_noise(T, 4096, seed=80 + T)
    x[:2, 1024:2048] = 0.0                                  # a silent pair in frame 3: powers of exactly zero
    rows, P = device_rows(gab, x, H), device_rows(gab, x, H, "power")
    assert rows.shape[:3] == P.shape == (8, T, BINS) and not P[3, :2].any() and (np.delete(P, 3, axis=0) > 0).all()
    plan = gab.DenoisePlan(T, 512, H)
    plan.set_params(up(np.zeros((T, 3), F32)))              # floor 0, att = rel = 0: the mask is the verdict
    for f in range(8):
        plan.set_thresholds(up(P[f]))                       # thr = P: strict, so every bin shuts
        out = host(plan.process_rows(up(rows[f:f + 1])))
        assert not out.any() and not host(plan.state()[2]).any(), f
        plan.set_thresholds(up(np.where(P[f] > 0, np.nextafter(P[f], F32(0.0)), F32(0.0))))
        out = host(plan.process_rows(up(rows[f:f + 1])))    # one float below: every bin with a power opens
        assert same_bits(out[0], rows[f]), f
        assert same_bits(host(plan.state()[2]), (P[f] > 0).astype(F32)), f
    plan.close()


# ---- 4. it reduces noise ---------------------------------------------------------------------------------------------
def test_a_learnt_profile_removes_the_noise_and_keeps_the_tone(gab):
    T, H, total = 2, 256, 8192
    rng = np.random.default_rng(90)
    noise = (1e-3 * rng.standard_normal((T, total))).astype(F32)
    learn = (1e-3 * rng.standard_normal((T, total))).astype(F32)
    tone = (0.5 * np.sin(2.0 * np.pi * 100 * np.arange(total) / N))[None, :]
    x = (tone + noise).astype(F32)
    thr = host(gab.denoise_thresholds(dev(device_rows(gab, learn, H, "power")[4:]), 20.0))      # whole windows of noise
    # a condition on the inputs: no bin of the signal's own noise exceeds its threshold (at 100 times the mean of an
    # exponentially distributed power none should)
    S = st.window_sum(st.window_hann())
    Pn = st.powers(rt.as_complex(rt.analyse(noise, H)), S)
    assert (Pn <= thr[None]).all() and (thr > 0).all()
    rows = device_rows(gab, x, H)[4:]                       # the frames that lie inside the stream: the tone is steady
    plan = gab.DenoisePlan(T, 512, H)
    set_tables([plan], thr, np.zeros((T, 3), F32))
    out = host(plan.process_rows(up(rows)))
    plan.close()
    quiet = np.ones(BINS, bool)
    quiet[97:104] = False
    assert len(rows) == 28 and not out[:, :, quiet].any()
    assert same_bits(out[:, :, 100], rows[:, :, 100]) and (np.abs(rows[:, :, 100, :]).max(axis=-1) > 100).all()
    assert np.abs(rows[:, :, quiet]).max() > 0


# ---- 5. accuracy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(256, 512), (512, 512), (100, 512)])
def test_fused_output_is_within_4_times_the_twin_chains_error_of_the_float64_chain(gab, H, B):
    """Per pair, against the float64 chain with the same tables; the inputs keep every float64 power a factor 1 +- 1e-3
    away from its threshold, so no decision can flip.  Measured ratios: profiles/r27_denoise.txt."""
    T, total = 3, 4096
    x, thr, params = dt.accuracy_case(T, total, H, seed=500 + H)
    ref, P64 = dt.truth64(x, H, thr, params)
    assert dt.clear_of_thresholds(P64, thr, 1e-3)
    assert (P64 > thr[None]).any(axis=0).all() and (P64 < thr[None]).any(axis=0).all()
    twin = dt.Denoiser(T, total, H)
    set_tables([twin.gate], thr, params)
    e_twin = dt.pair_err(dt.stream_of(twin.process(x[None])), ref)
    plan = gab.DenoisePlan(T, B, H)
    set_tables([plan], thr, params)
    y = np.concatenate([host(plan.process(dev(b))) for b in st.blocks(x, B)], axis=1)
    plan.close()
    e_gpu = dt.pair_err(y, ref)
    print("\ndenoise accuracy H %d e_twin %s e_gpu %s ratio %.2f" % (H, e_twin, e_gpu, (e_gpu / e_twin).max()))
    assert (e_twin > 0).all() and (e_twin <= 8e-6).all()
    assert (e_gpu <= FACTOR * e_twin).all(), e_gpu / e_twin
    assert not y[:, :H].any()


# ---- 6. the edges of float32 -----------------------------------------------------------------------------------------
def test_the_gain_decays_through_the_subnormals_to_zero(gab):
    T, H, B, nb = 3, 32, 64, 112                            # 224 frames: 150 to reach zero, 32 more to flush the delay
    x = unit_noise(T, nb * B, seed=95)
    bl = st.blocks(x, B)
    thr = np.full((T, BINS), np.inf, F32)                   # always shut
    thr[1, 200:] = 0.0                                      # but for half a track, which stays open
    params = np.tile(np.array([0.0, 0.0, 0.5], F32), (T, 1))
    fused, comp, probe, twin = gab.DenoisePlan(T, B, H), Composed(gab, T, B, H), gab.DenoisePlan(T, B, H), dt.Gate(T)
    set_tables([fused, comp.gate, probe, twin], thr, params)
    rows = device_rows(gab, x, H)                           # the bits the composition's analyser writes
    k, frames, seen_subnormal = 0, 0, False
    for n in [16] * 7:
        k, y = drive(fused, comp, bl, [n], first=k)
        f = rt.count(0, k * B, H)
        want = twin.take(rows[frames:f])
        assert same_bits(host(probe.process_rows(up(rows[frames:f]))), want), f     # m * re through the subnormals
        mask = host(fused.state()[2])
        assert same_bits(mask, twin.mask) and same_bits(host(probe.state()[2]), twin.mask), f
        assert same_bits(mask[0], np.full(BINS, 2.0 ** -f if f <= 149 else 0.0, F32)), f
        seen_subnormal = seen_subnormal or 0 < mask[0, 0] < 2.0 ** -126
        frames = f
    assert seen_subnormal and frames == 224 and not mask[0].any() and not mask[2].any() and (mask[1, 200:] == 1.0).all()
    # track 2 stands alone and is silent by now; track 0 is shut beside a partner that is half open, so it holds the
    # pair's rounding error (four times the round trip's 4e-6 at unit level at the most) and nothing else
    assert not y[2, -B:].any() and y[1, -B:].any() and np.abs(y[0, -B:]).max() <= FACTOR * 4e-6
    for p in (fused, comp, probe):
        p.close()


@pytest.mark.parametrize("H,B", [(256, 512), (100, 64)])
def test_a_nan_and_an_infinity_stay_in_their_pair_and_their_frames_and_leave_the_mask_finite(gab, H, B):
    T, total = 9, 6144
    nb = total // B
    x = unit_noise(T, total, seed=97)
    thr, params = dt.seeded_tables(T, 98, LEVEL)
    params[:, 0] = np.maximum(params[:, 0], 0.25)

    def run(xs):
        plan = gab.DenoisePlan(T, B, H)
        set_tables([plan], thr, params)
        outs, masks = [], []
        for k in range(0, nb, 4):
            outs.append(dt.stream_of(host(plan.process_batch(dev(st.blocks(xs, B)[k:k + 4])))))
            masks.append(host(plan.state()[2]))
        hist, acc = (host(s) for s in plan.state()[:2])
        plan.close()
        return np.concatenate(outs, axis=1), masks, hist, acc

    base, bmasks, bhist, bacc = run(x)
    assert np.isfinite(base).all()
    for t, s0, v in ((0, 700, np.nan), (T - 1, 1500, np.inf), (3, 1023, -np.inf)):
        xs = x.copy()
        xs[t, s0] = v
        y, masks, hist, acc = run(xs)
        js = [j for j in range(1, total // H + 1) if j * H - N <= s0 < j * H]
        struck = np.zeros(total, bool)
        for j in js:
            struck[j * H:j * H + N] = True                  # frame j's samples are outputs jH .. jH + N
        assert struck[:total].any() and not struck[-B:].any()
        pair = [s for s in (t & ~1, (t & ~1) + 1) if s < T]
        for m in masks:
            assert np.isfinite(m).all() and (m >= 0).all() and (m <= 1).all()
        for s in range(T):
            if s in pair:
                assert np.isfinite(y[s, ~struck]).all() and not np.isfinite(y[s, struck]).all(), (t, s)
                assert same_bits(y[s, :js[0] * H], base[s, :js[0] * H]), (t, s)
                assert np.isfinite(acc[s]).all() and np.isfinite(hist[s]).all(), (t, s)
            else:
                assert same_bits(y[s], base[s]) and same_bits(acc[s], bacc[s]) and same_bits(hist[s], bhist[s]), (t, s)
                assert all(same_bits(m[s], bm[s]) for m, bm in zip(masks, bmasks)), (t, s)
        assert not np.isfinite(y[t, struck]).any(), t       # the struck track's own samples: every one


# ---- 7. the rest -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [9, 17])
def test_a_silent_pair_gives_zeros_and_a_pair_aligned_shard_gives_its_tracks_bits(gab, T):
    H, B, nb = 100, 100, 48
    x = unit_noise(T, nb * B, seed=100 + T)
    silent = [2, 3] + ([10, 11] if T > 11 else [])
    x[silent] = 0.0
    thr, params = dt.seeded_tables(T, 110 + T, LEVEL)
    whole = gab.DenoisePlan(T, B, H)
    set_tables([whole], thr, params)
    want = host(whole.process_batch(dev(st.blocks(x, B))))
    wstate = [host(s) for s in whole.state()[:3]]
    whole.close()
    assert not want[:, silent].any() and want[:, 0].any() and want[:, T - 1].any()
    for lo, hi in ((0, 2), (2, 8), (6, T)):
        shard = gab.DenoisePlan(hi - lo, B, H)
        set_tables([shard], thr[lo:hi], params[lo:hi])
        got = host(shard.process_batch(dev(st.blocks(x[lo:hi], B))))
        assert same_bits(got, want[:, lo:hi]), (lo, hi)
        for s, w in zip(shard.state()[:3], wstate):
            assert same_bits(host(s), w[lo:hi]), (lo, hi)
        shard.close()


def test_calls_of_one_sample_and_a_batch_longer_than_the_history(gab):
    T, H = 3, 32
    x = unit_noise(T, 70 + 1100, seed=120)
    bl = st.blocks(x, 1)
    thr, params = dt.seeded_tables(T, 121, LEVEL)
    fused, comp = gab.DenoisePlan(T, 1, H), Composed(gab, T, 1, H)
    set_tables([fused, comp.gate], thr, params)
    k, _ = drive(fused, comp, bl, [1] * 70)                 # 70 calls of one sample: two take a frame
    assert fused.state()[3] == 70 % H
    k, _ = drive(fused, comp, bl, [1100], first=k)          # the new history holds nothing of the old
    assert k == 1170 and same_bits(host(fused.state()[0]), x[:, -1023:])
    fused.close()
    comp.close()


def test_prepare_launch_and_a_captured_graph_replay_to_the_bits_of_plain_calls(gab):
    import torch
    T, B, H = 9, 512, 256
    bl = st.blocks(unit_noise(T, 8 * B, seed=130), B)
    thr, params = dt.seeded_tables(T, 131, LEVEL)
    plan = gab.DenoisePlan(T, B, H)
    set_tables([plan], thr, params)
    want = [host(plan.process(dev(b))) for b in bl]
    wmask = host(plan.state()[2])
    plan.reset()
    xin, out = torch.zeros(T * B, device="cuda"), torch.zeros((T, B), device="cuda")
    args = plan.prepare(xin, out)
    for k in range(2):                                      # prepare / launch
        xin.copy_(dev(bl[k].ravel()))
        plan.launch(args)
        torch.cuda.synchronize()
        assert same_bits(host(out), want[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        a = plan.prepare(xin, out)
        with torch.cuda.graph(graph, stream=side):
            plan.launch(a)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k in range(2, 8):
        xin.copy_(dev(bl[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(host(out), want[k]), k
    assert same_bits(host(plan.state()[2]), wmask)
    del graph
    plan.close()
    odd = gab.DenoisePlan(T, 100, 96)
    with pytest.raises(ValueError, match="DenoisePlan.prepare: hop 96 does not divide bufsize 100"):
        odd.prepare(torch.zeros(T * 100, device="cuda"), torch.zeros(T * 100, device="cuda"))
    odd.close()


def test_refusals_each_with_its_text(gab):
    import torch
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()

    def refused(rc, text):
        assert rc == bad and text in lib.gab_last_error().decode(), (rc, lib.gab_last_error())

    for hop in (31, 1025, 0, -5):
        refused(lib.gab_dn_create(ctypes.byref(h), 4, 512, hop), "gab_dn_create: hop must be 32..1024")
        assert not h.value
    refused(lib.gab_dn_create(ctypes.byref(h), 0, 512, 512), "tracks and bufsize must be > 0")
    refused(lib.gab_dn_create(ctypes.byref(h), 4, 0, 512), "tracks and bufsize must be > 0")
    refused(lib.gab_dn_create(ctypes.byref(h), (1 << 26) + 1, 512, 512), "more than 2^23 workgroups")
    refused(lib.gab_dn_create(None, 4, 512, 512), "null plan pointer")
    assert not h.value

    T, B, H = 3, 512, 256
    bl = st.blocks(unit_noise(T, 6 * B, seed=140), B)
    thr, params = dt.seeded_tables(T, 141, LEVEL)
    plan, comp = gab.DenoisePlan(T, B, H), Composed(gab, T, B, H)
    set_tables([plan, comp.gate], thr, params)
    k, _ = drive(plan, comp, bl, [1, 1])
    # the tables: the first bad value is named and the table is kept
    for i, v in ((5, np.nan), (BINS + 7, -1.0), (3 * BINS - 1, -np.inf)):
        t = thr.copy().ravel()
        t[i] = v
        t[min(i + 3, t.size - 1)] = np.nan
        with pytest.raises(gab.GabError, match="gab_dn_set_thresholds: track %d bin %d \\(threshold\\) must be >= 0 or "
                           "\\+inf, not a NaN; the plan keeps its thresholds" % (i // BINS, i % BINS)):
            plan.set_thresholds(up(t.reshape(T, BINS)))
    with pytest.raises(gab.GabError, match="track 2 bin 4 \\(threshold\\)"):
        plan.set_thresholds(up(np.array([0.0] * 4 + [np.nan] + [0.0] * (BINS - 5), F32)), 2)
    for field, values in {0: (np.nan, -1.0, 1.5, np.inf), 1: (np.nan, -0.5, 1.0, np.inf), 2: (np.nan, -0.5, 1.0, 2.0)}.items():
        for v in values:
            p = params.copy()
            p[1, field] = v
            p[2, 0] = np.nan
            with pytest.raises(gab.GabError) as e:
                plan.set_params(up(p))
            assert "gab_dn_set_params: " + dt.param_refusal(3 + field) in str(e.value), (field, v)
    with pytest.raises(gab.GabError, match="track 2 field 1 \\(att\\) must be within \\[0, 1\\)"):
        plan.set_params(up(np.array([0.5, 1.0, 0.5], F32)), 2)
    for first, n in ((-1, 1), (3, 1), (1, 3), (0, 0)):
        tt = torch.zeros(4 * BINS, device="cuda")
        ptr = ctypes.c_void_p(tt.data_ptr())
        refused(lib.gab_dn_set_thresholds(plan._h, ptr, first, n, None), "the track range is outside the plan")
        refused(lib.gab_dn_set_params(plan._h, ptr, first, n, None), "the track range is outside the plan")
    # the windows: both are kept
    w, g = st.window_hann(), rt.dual_window(st.window_hann(), H)
    for n, v in ((700, np.nan), (0, np.inf), (1023, -np.inf)):
        s = w.copy()
        s[n] = v
        s[min(n + 1, 1023)] = v
        with pytest.raises(gab.GabError, match="analysis window value %d is not finite; the plan keeps its windows" % n):
            plan.set_windows(dev(s), dev(g * 2))
        s = g.copy()
        s[n] = v
        with pytest.raises(gab.GabError, match="synthesis window value %d is not finite; the plan keeps its windows" % n):
            plan.set_windows(dev(w * 2), dev(s))
    with pytest.raises(gab.GabError, match="the analysis window's sum is zero; the plan keeps its windows"):
        plan.set_windows(dev(np.concatenate([np.ones(512, F32), -np.ones(512, F32)])), dev(g * 2))
    # pointers
    x = torch.zeros(2 * T * B + 8, device="cuda")
    xp, op = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr() + 4 * T * B)
    for args in ((plan._h, None, op), (plan._h, xp, None), (None, xp, op)):
        refused(lib.gab_dn_process(*args, None), "gab_dn_process: null pointer")
        refused(lib.gab_dn_process_batch(*args, 1, None), "gab_dn_process_batch: null pointer")
        refused(lib.gab_dn_process_rows(*args, 1, None), "gab_dn_process_rows: null pointer")
    refused(lib.gab_dn_process_batch(plan._h, xp, op, 0, None), "n_buffers must be > 0")
    refused(lib.gab_dn_process_batch(plan._h, xp, op, (1 << 22) - 1, None), "n_buffers * bufsize must be below 2^31 - 1024")
    for shift in (0, 4, 4 * T * B - 4):
        refused(lib.gab_dn_process(plan._h, xp, ctypes.c_void_p(x.data_ptr() + shift), None), "gab_dn_process: d_in and d_out overlap")
    refused(lib.gab_dn_process(plan._h, ctypes.c_void_p(x.data_ptr() + 4 * T * B - 4), xp, None), "d_in and d_out overlap")
    r = torch.zeros(2 * T * BINS * 2 + 8, device="cuda")
    rp, rq = ctypes.c_void_p(r.data_ptr()), ctypes.c_void_p(r.data_ptr() + 8 * T * BINS)
    refused(lib.gab_dn_process_rows(plan._h, ctypes.c_void_p(r.data_ptr() + 4), rq, 1, None), "d_rows_in must lie on an 8-byte boundary")
    refused(lib.gab_dn_process_rows(plan._h, rp, ctypes.c_void_p(r.data_ptr() + 8 * T * BINS + 4), 1, None),
            "d_rows_out must lie on an 8-byte boundary")
    for shift in (8, 8 * T * BINS - 8):
        refused(lib.gab_dn_process_rows(plan._h, rp, ctypes.c_void_p(r.data_ptr() + shift), 1, None),
                "d_rows_in and d_rows_out overlap in part")
        refused(lib.gab_dn_process_rows(plan._h, ctypes.c_void_p(r.data_ptr() + shift), rp, 1, None),
                "d_rows_in and d_rows_out overlap in part")
    refused(lib.gab_dn_process_rows(plan._h, rp, rq, -1, None), "n_frames must be >= 0")
    refused(lib.gab_dn_set_thresholds(plan._h, None, 0, 1, None), "gab_dn_set_thresholds: null pointer")
    refused(lib.gab_dn_set_params(None, rp, 0, 1, None), "gab_dn_set_params: null pointer")
    refused(lib.gab_dn_set_windows(plan._h, rp, None, None), "gab_dn_set_windows: null pointer")
    refused(lib.gab_dn_set_windows(plan._h, None, rp, None), "gab_dn_set_windows: null pointer")
    refused(lib.gab_dn_state(plan._h, None, None, None, None), "gab_dn_state: null pointer")
    refused(lib.gab_dn_tables(plan._h, None, None), "gab_dn_tables: null pointer")
    refused(lib.gab_dn_latency(plan._h, None), "gab_dn_latency: null pointer")
    refused(lib.gab_dn_reset(None, None), "gab_dn_reset: null pointer")
    refused(lib.gab_dn_destroy(None), "gab_dn_destroy: null pointer")
    with pytest.raises(ValueError, match="whole frames"):
        plan.process_rows(torch.zeros(T * BINS * 2 + 2, device="cuda"))
    # every refusal left the plan as it was: tables, windows and state
    t, p = plan.tables()
    assert same_bits(host(t), thr) and same_bits(host(p), params)
    drive(plan, comp, bl, [1, 2], first=k)
    plan.close()
    comp.close()


@pytest.mark.parametrize("H,B", [(100, 64), (512, 512), (1024, 1536)])
def test_state_after_create_and_reset_and_an_accepted_set_of_windows(gab, H, B):
    T = 3
    nb = -(-3072 // B)
    bl = st.blocks(unit_noise(T, nb * B, seed=150 + H), B)
    thr, params = dt.seeded_tables(T, 151, LEVEL)
    plan = gab.DenoisePlan(T, B, H)
    t, p = plan.tables()
    assert not host(t).any() and same_bits(host(p), dt.default_params(T))
    hist, acc, mask, phase = plan.state()
    assert not host(hist).any() and not host(acc).any() and (host(mask) == 1.0).all() and phase == 0
    assert hist.shape == (T, 1023) and acc.shape == (T, 1024) and mask.shape == (T, BINS)
    set_tables([plan], thr, params)
    first = host(plan.process_batch(dev(bl)))
    plan.process_batch(dev(bl[:3]))                         # leaves a phase, an accumulator and a mask behind
    plan.reset()
    hist, acc, mask, phase = plan.state()
    assert not host(hist).view(np.uint32).any() and not host(acc).view(np.uint32).any() and phase == 0
    assert same_bits(host(mask), np.ones((T, BINS), F32))
    t, p = plan.tables()
    assert same_bits(host(t), thr) and same_bits(host(p), params)          # the tables stay
    assert same_bits(host(plan.process_batch(dev(bl))), first)
    # other windows: the composition under the same windows, and P scaled by the new sum
    w = (st.window_hann() * np.linspace(0.5, 1.5, N)).astype(F32)
    g = host(gab.synthesis_window(dev(w), min(H, 512)))
    comp = Composed(gab, T, B, H)
    plan.reset()
    plan.set_windows(dev(w), dev(g))
    comp.gate.set_windows(dev(w), dev(g))
    comp.spec.set_window(dev(w))
    comp.resyn.set_window(dev(g))
    set_tables([comp.gate], thr, params)
    drive(plan, comp, bl, [1, nb - 1])
    plan.close()
    comp.close()
