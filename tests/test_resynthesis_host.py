"""The resynthesis plan's restatement (resynthesis_twin.py) held without a GPU: the counts against brute force, any cut
of a stream against the whole stream bit for bit (outputs and accumulator), the order of the sum, the dual window in
float64 and through the float32 chain analyser twin -> resynthesis twin, known answers, the rule on bins 0 and 512, the
window rule, and the twin's own error on the inputs that test_resynthesis_gpu.py uses."""
import math

import numpy as np
import pytest

import conv_pair_twin as tw
import resynthesis_twin as rt
import spectrum_twin as st

N, BINS = rt.N, rt.BINS
F32 = np.float32
GRID_B, GRID_H = (1, 64, 100, 512, 1536), (32, 100, 256, 512, 1024)
DUAL_H = (32, 100, 256, 300, 512)
TRACKS = [1, 2, 3, 9, 17]


def gab_ops():
    import gpuaudiobench_amd
    return gpuaudiobench_amd


def unit_noise(T, total, seed):
    """[T, total] float32, uniform in [-1, 1): unit-level noise."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (T, total)).astype(F32)


def random_frames(F, T, seed):
    return np.random.default_rng(seed).standard_normal((F, T, N)).astype(F32)


def by_calls(adder, u, sizes):
    """The frames u [F, T, 1024] through `adder` in calls of sizes[i] buffers: (outputs [T, total], counts)."""
    out, calls, f = [], [], 0
    for n in sizes:
        k = adder.count(n)
        blk = adder.take(u[f:f + k], n)
        out.append(blk.transpose(1, 0, 2).reshape(adder.T, n * adder.B))
        calls.append(k)
        f += k
    assert f == len(u)
    return np.concatenate(out, axis=1), calls


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", GRID_H + (96, 1000))
@pytest.mark.parametrize("B", GRID_B)
def test_counts_against_brute_force(B, H):
    n = max(40, 3 * H // B + 3)
    ends = [j * H for j in range(1, n * B // H + 2)]
    brute = [sum(1 for e in ends if k * B < e <= (k + 1) * B) for k in range(n)]
    assert rt.counts(B, H, 0, n) == brute
    assert gab_ops().ResynthesisPlan.counts(B, H, 0, n) == brute
    assert gab_ops().ResynthesisPlan.counts(B, H, 7, n - 7) == brute[7:]
    a = rt.Adder(1, B, H, np.ones(N, F32))
    for m in (1, 2, 5, 1, 3):                             # the carried position gives the same counts
        k = a.count(m)
        assert k == rt.count(a.p, m * B, H) <= rt.capacity(B, H, m)
        a.take(np.zeros((k, 1, N), F32), m)
    assert rt.frame_ends(0, n * B, H) == [e for e in ends if e <= n * B]


# ---- cuts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", GRID_H)
def test_any_cut_of_a_stream_gives_the_outputs_and_the_accumulator_of_the_whole_stream(H):
    T, total = 3, 3072
    ends = rt.frame_ends(0, total, H)
    u = random_frames(len(ends), T, seed=H)
    g = rt.dual_window(st.window_hann(), H) if H < N else np.ones(N, F32)
    every, _ = rt.overlap_add(u, ends, g, total)
    assert not every[:, :H].any() and every[:, H:].any()   # the first H outputs are zeros, the next are not
    for B in GRID_B:
        nb = total // B                                    # whole buffers: 3000 samples at B = 100
        k = rt.count(0, nb * B, H)
        whole, tail = rt.overlap_add(u[:k], ends[:k], g, nb * B)
        assert same_bits(whole, every[:, :nb * B])         # a later frame touches no earlier output
        a = rt.Adder(T, B, H, g)
        got, calls = by_calls(a, u[:k], [1] * nb)
        assert calls == rt.counts(B, H, 0, nb)
        assert same_bits(got, whole) and same_bits(a.acc, tail) and a.p == nb * B, B
        a.reset()
        assert not a.acc.any() and a.p == 0
        sizes, left = [], nb
        for m in (1, 3, 2, 5, 1) * (nb // 12 + 1):
            if left == 0:
                break
            sizes.append(min(m, left))
            left -= sizes[-1]
        got, _ = by_calls(a, u[:k], sizes)
        assert same_bits(got, whole) and same_bits(a.acc, tail), B
    one = rt.Adder(T, total, H, g)                          # the whole stream as one buffer
    whole, tail = rt.overlap_add(u, ends, g, total)
    assert same_bits(one.take(u)[0], whole) and same_bits(one.acc, tail)


def test_the_accumulators_first_slot_is_complete_and_a_call_without_a_frame_only_shifts():
    T, B, H = 2, 100, 512
    u = random_frames(4, T, seed=3)
    a = rt.Adder(T, B, H, np.ones(N, F32))
    outs = []
    for k in range(20):
        before, c = a.acc.copy(), a.count()
        blk = a.take(u[:c] if c else np.zeros((0, T, N), F32))[0]
        if c == 0:
            assert same_bits(blk, before[:, :B]) and same_bits(a.acc[:, :N - B], before[:, B:])
            assert not a.acc[:, N - B:].any()
        outs.append(blk)
        nxt = a.acc[:, 0].copy()
        b2 = rt.Adder(T, B, H, np.ones(N, F32))
        b2.acc, b2.p = a.acc.copy(), a.p
        c2 = b2.count()
        assert same_bits(b2.take(random_frames(c2, T, seed=k))[0][:, 0], nxt)     # whatever comes, acc[0] goes out


# ---- the order of the sum --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 100, 256])
def test_the_ordered_sum_against_fsum_within_the_bound_of_an_ordered_sum(H):
    T, total = 2, 2048
    ends = rt.frame_ends(0, total, H)
    u = random_frames(len(ends), T, seed=50 + H)
    g = rt.dual_window(st.window_hann(), H)
    y, _ = rt.overlap_add(u, ends, g, total)
    v = (g[None, None, :] * u).astype(F32)
    for t in range(T):
        for o in range(N, total, 37):
            a = o - N
            terms = [float(v[i, t, a - (e - N)]) for i, e in enumerate(ends) if e - N <= a < e]
            assert len(terms) == -(-N // H) or len(terms) == N // H
            bound = st.ordered_sum_bound([abs(x) for x in terms])                 # each addition rounds at most sum |v|
            assert abs(float(y[t, o]) - math.fsum(terms)) <= bound, (t, o)
            acc = F32(0.0)
            for x in terms:
                acc = F32(acc + F32(x))
            assert acc == y[t, o]                                                 # ascending j from +0.0f, to the bit


# ---- the dual window -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", DUAL_H)
def test_the_dual_window_sums_to_one_with_hann_in_float64(H):
    w = st.window_hann().astype(np.float64)
    g = rt.dual_window64(w, H)
    for r in range(H):
        assert abs(sum(w[i] * g[i] for i in range(r, N, H)) - 1.0) <= 1e-12, r
    assert same_bits(rt.dual_window(st.window_hann(), H), g.astype(F32))
    import torch
    got = gab_ops().synthesis_window(torch.from_numpy(st.window_hann()), H)
    assert got.dtype == torch.float32 and same_bits(got.numpy(), rt.dual_window(st.window_hann(), H))
    assert same_bits(gab_ops().synthesis_window(list(st.window_hann()), H).numpy(), got.numpy())


def test_the_dual_window_grows_ill_conditioned_towards_hop_1024():
    w = st.window_hann()
    peaks = [float(np.abs(rt.dual_window(w, H)).max()) for H in (256, 512, 700, 1000, 1023)]
    assert np.allclose(peaks, [0.6667, 1.207, 2.586, 430.3, 1.062e5], rtol=1e-3), peaks
    g = rt.dual_window(w, 1024)
    assert g[0] == 0.0 and np.isfinite(g).all()            # Hann's zero cannot be undone: sample 0 of a frame is lost
    other = np.sqrt(w.astype(np.float64)).astype(F32)       # any analysis window: root-Hann at hop 512 is its own dual
    assert np.abs(rt.dual_window(other, 512) - other).max() <= 2e-7
    with pytest.raises(ValueError, match="hop must be 32..1024"):
        gab_ops().synthesis_window(w, 31)
    with pytest.raises(ValueError, match="1024 values"):
        gab_ops().synthesis_window(w[:100], 512)


@pytest.mark.parametrize("H", DUAL_H)
def test_the_float32_chain_returns_unit_noise_delayed_by_1024_within_1e_6(H):
    """analyser twin -> resynthesis twin, both in float32, from sample 0 on.  Measured: 2.4e-7 to 3.6e-7."""
    T, B, total = 2, 512, 4096
    x = unit_noise(T, total, seed=H)
    u = rt.frames_f32(rt.analyse(x, H))
    a = rt.Adder(T, B, H, rt.dual_window(st.window_hann(), H))
    y, _ = by_calls(a, u, [1] * (total // B))
    err = float(np.abs(y[:, N:].astype(np.float64) - x[:, :total - N]).max())
    print("\nresynthesis twin chain H %d err %.3g head %.3g" % (H, err, np.abs(y[:, :N]).max()))
    assert err <= 1e-6
    assert not y[:, :H].any() and np.abs(y[:, :N]).max() <= 1e-6          # y at negative indices: rounding level


# ---- known answers ---------------------------------------------------------------------------------------------------
def test_known_answers_dc_a_single_bin_and_the_all_ones_window():
    T, H = 3, 1024
    g = rt.dual_window(st.window_hann(), 512)
    n = np.arange(N)
    rows = np.zeros((1, T, BINS, 2), F32)
    rows[0, 0, 0, 0] = 1024 * 0.75                         # a constant 0.75
    rows[0, 1, 37, 0] = 512 * 0.5                          # 0.5 cos(2 pi 37 n / N)
    rows[0, 2, 512, 0] = 1024 * -0.25                      # -0.25 (-1)^n
    want = np.stack([np.full(N, 0.75), 0.5 * np.cos(2 * np.pi * 37 * n / N), -0.25 * np.where(n % 2 == 0, 1.0, -1.0)])
    assert np.abs(rt.truth(rows)[0] - want).max() <= 1e-12
    u = rt.frames_f32(rows)
    a = rt.Adder(T, 1024, H, g)
    first = a.take(u)[0]
    assert not first.any()                                 # the latency: nothing of frame 1 before output 1024
    out = a.take(np.zeros((1, T, N), F32))[0]
    assert np.abs(out - g[None, :] * want).max() <= 4e-7
    ones = rt.Adder(T, 1024, H, np.ones(N, F32))           # H = 1024 under all ones returns u itself
    r = random_frames(3, T, seed=8)
    ones.take(r[0:1])
    assert same_bits(ones.acc, r[0]) and same_bits(ones.take(r[1:2])[0], r[0]) and same_bits(ones.take(r[2:3])[0], r[1])


def test_the_imaginary_parts_of_bins_0_and_512_are_ignored():
    T = 3
    rows = rt.noise_rows(2, T, seed=4)
    clean = rows.copy()
    clean[..., 0, 1] = 0.0
    clean[..., 512, 1] = 0.0
    assert rows[..., 0, 1].any() and rows[..., 512, 1].any()
    assert same_bits(rt.frames_f32(rows), rt.frames_f32(clean))
    assert np.array_equal(rt.truth(rows), rt.truth(clean))
    spoilt = rows.copy()
    spoilt[..., 0, 1], spoilt[..., 512, 1] = np.nan, np.inf
    assert same_bits(rt.frames_f32(spoilt), rt.frames_f32(clean))


# ---- the window rule -------------------------------------------------------------------------------------------------
def test_the_window_rule_on_every_spoilt_field():
    g = rt.dual_window(st.window_hann(), 512)
    assert rt.bad_window(g) is None
    for n in (0, 1, 63, 64, 511, 1023):
        for v in (np.nan, np.inf, -np.inf):
            s = g.copy()
            s[n] = v
            assert rt.bad_window(s) == n
    s = g.copy()
    s[[700, 3]] = np.nan
    assert rt.bad_window(s) == 3                           # the first
    assert rt.bad_window(np.zeros(N, F32)) is None         # no rule on a sum
    assert rt.bad_window(np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(F32)) is None
    assert rt.bad_window(np.full(N, np.finfo(F32).max, F32)) is None


# ---- the twin's own error --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TRACKS)
def test_the_twins_error_is_within_its_cap(T):
    """c_twin on noise rows at conv_pair_twin.levels(T): inside (0, 1e-6], so four times it is a bound on the kernel
    that means something."""
    rows = rt.noise_rows(4, T, seed=200 + T)
    c, level = rt.figures(rt.frames_f32(rows), rt.truth(rows))
    c_twin = tw.c_max(c)
    print("\nresynthesis twin T %d c_twin %.3g" % (T, c_twin))
    assert 0 < c_twin <= 1e-6
    assert (level > 0).all()                               # levels(T) has silent tracks but no silent pair
