"""The resample plan on the device against its restatement (tests/test_resample_host.py): whole rows with the zero
fill, the counts and state(), bit for bit.

Which path a shape takes: 1, 3, 65 and 130 tracks are below, across and beyond a 64-track workgroup; bufsize 1, 7 and 31
are below K-1 (the history is shifted, not replaced), 64 is one chunk, 100 and 513 end in a short chunk; 1/2 at bufsize 1
has buffers without an output; 2/1 and 3/2 put more outputs into a chunk than one turn of the output tile holds only
at a higher ratio, so (16, 1) is here for that; K = 6 takes the other row pitch (K mod 4 = 2), K = 256 the largest
tile (more dynamic LDS than the default limit, a history of four 64-column passes)."""
import functools

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_resample_host import F32, Twin, default_taps, noise, reduced, resample_taps32

pytestmark = pytest.mark.gpu

#          up  down taps tracks bufsize buffers
SHAPES = [(160, 147, None, 3, 7, 23),       # period 21
          (160, 147, None, 130, 513, 3),
          (160, 147, None, 65, 64, 4),
          (147, 160, None, 3, 31, 162),     # period 160, K = 40 > bufsize
          (147, 160, None, 65, 100, 10),    # period 8
          (2, 1, None, 1, 1, 8),
          (2, 1, None, 3, 31, 4),
          (1, 2, None, 130, 1, 6),          # K = 64, every other buffer without an output
          (1, 2, None, 1, 513, 3),
          (3, 2, 6, 3, 100, 4),
          (1, 1, None, 65, 64, 3),
          (4, 6, None, 3, 7, 5),
          (16, 1, 8, 3, 100, 2),            # 1024 outputs of a 64-sample chunk
          (1, 1, 256, 3, 100, 3),
          # positions the ratios above do not reach (tests/test_resample_host.py, TAPS)
          (2, 5, 16, 66, 100, 5),           # M/L = 2 and M mod L = 1: both increments at once
          (5, 2, 6, 66, 65, 3),             # M mod L = 2 of 5 at the row pitch of K mod 4 = 2; counts 163, 162, 163
          (7, 3, 12, 130, 1, 9),            # bufsize 1: counts 3, 2, 2, period 3
          (3, 200, 8, 3, 64, 12),           # M/L = 66: one output per 64-sample buffer at most, period 25
          (3, 64, 64, 3, 65, 4),            # M/L = 21, M mod L = 1, period 64
          (1, 65, 8, 65, 64, 4),            # one output per buffer, a sample later each time; period 65
          (1, 1024, 4, 3, 100, 24),         # 21 of 24 buffers without an output
          (64, 1, 256, 2, 7, 3),            # the largest table and tile; 448 outputs of a 7-sample chunk
          (1000, 1024, 16, 3, 513, 2)]      # reduces to 125/128, period 128


def ident(s):
    return "x".join("d" if v is None else str(v) for v in s)


def same(a, b):
    """Bit for bit; two NaNs count as the same."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@functools.lru_cache(maxsize=None)
def case(shape):
    """(xs [n][T][B] with a NaN and an infinity in the last track, rows [n][T][out_capacity], counts, history)."""
    up, down, K, T, B, n = shape
    xs = noise(n, T, B, seed=up + T + B)
    xs[min(1, n - 1), T - 1, B // 2] = np.nan
    xs[n - 1, T - 1, 0] = np.inf
    xs.setflags(write=False)
    twin = Twin(T, B, up, down, K)
    out = [twin.process(x) for x in xs]
    rows = np.stack([r for r, _ in out])
    rows.setflags(write=False)
    return xs, rows, [c for _, c in out], twin.hist.copy(), twin.k


def make(gab, shape):
    up, down, K, T, B, _ = shape
    return gab.ResamplePlan(T, B, up, down, K)


def run(plan, xs):
    rows, counts = [], []
    for x in xs:
        out, n = plan.process(dev(x.reshape(-1)))
        rows.append(host(out))
        counts.append(n)
    return np.stack(rows), counts


@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_single_calls_against_the_restatement(gab, shape):
    up, down, K, T, B, n = shape
    xs, rows, counts, hist, k = case(shape)
    plan = make(gab, shape)
    L, M = reduced(up, down)
    assert (plan.up, plan.down) == (L, M) and plan.ntaps == (K or default_taps(up, down))
    assert plan.out_capacity == rows.shape[2] and plan.latency == plan.ntaps // 2
    assert plan.period == M // np.gcd(B * L, M)
    assert same(host(plan.taps()), resample_taps32(up, down, plan.ntaps))
    x0 = dev(xs[0].reshape(-1))
    before = host(x0).copy()
    out0, n0 = plan.process(x0)
    assert same(host(x0), before)                                            # the input is only read
    got, got_counts = run(plan, xs[1:])
    got = np.concatenate([host(out0)[None], got])
    assert [n0] + got_counts == counts == gab.ResamplePlan.counts(B, up, down, 0, n)
    assert same(got, rows)
    h, kk = plan.state()
    assert same(host(h), hist) and kk == k == n % plan.period
    plan.close()


def test_four_sixths_reports_two_thirds(gab):
    plan = gab.ResamplePlan(3, 7, 4, 6)
    assert (plan.up, plan.down, plan.ntaps, plan.out_capacity, plan.period) == (2, 3, 48, 5, 3)
    plan.close()


@pytest.mark.parametrize("shape,cut", [((160, 147, None, 3, 7, 23), 12),     # the second launch crosses the period
                                       ((147, 160, None, 65, 100, 10), 3),
                                       ((1, 2, None, 130, 1, 6), 1),
                                       ((160, 147, None, 130, 513, 3), 2),
                                       ((2, 5, 16, 66, 100, 5), 2),
                                       ((5, 2, 6, 66, 65, 3), 1),
                                       ((7, 3, 12, 130, 1, 9), 4),          # across the period
                                       ((3, 200, 8, 3, 64, 12), 5),
                                       ((3, 64, 64, 3, 65, 4), 1),
                                       ((1, 65, 8, 65, 64, 4), 3),
                                       ((1, 1024, 4, 3, 100, 24), 11),      # both launches start between two outputs
                                       ((64, 1, 256, 2, 7, 3), 2),
                                       ((1000, 1024, 16, 3, 513, 2), 1)], ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_batch_equals_single_calls(gab, shape, cut):
    xs, rows, counts, hist, k = case(shape)
    plan = make(gab, shape)
    a, ca = plan.process_batch(dev(xs[:cut].reshape(-1)))
    b, cb = plan.process_batch(dev(xs[cut:].reshape(-1)))
    assert ca + cb == counts
    assert same(np.concatenate([host(a), host(b)]), rows)
    h, kk = plan.state()
    assert same(host(h), hist) and kk == k
    plan.close()


def test_a_shard_of_tracks_has_the_full_plans_bits(gab):
    shape = (160, 147, None, 130, 513, 3)
    xs, rows, counts, hist, _ = case(shape)
    part = gab.ResamplePlan(66, 513, 160, 147)
    got, got_counts = run(part, xs[:, 64:130])
    assert got_counts == counts and same(got, rows[:, 64:130])
    assert same(host(part.state()[0]), hist[64:130])
    part.close()


@pytest.mark.parametrize("shape", [(160, 147, None, 65, 64, 4), (147, 160, None, 65, 100, 10), (2, 1, None, 3, 31, 4)],
                         ids=ident)
def test_input_and_output_offset_by_one_float(gab, shape):
    import torch
    up, down, K, T, B, n = shape
    xs, rows, counts, _, _ = case(shape)
    plan = make(gab, shape)
    for i, x in enumerate(xs[:3]):
        src = torch.zeros(T * B + 1, dtype=torch.float32, device="cuda")
        dst = torch.full((T * plan.out_capacity + 2,), 7.0, dtype=torch.float32, device="cuda")
        src[1:].copy_(dev(x.reshape(-1)))
        assert src[1:].data_ptr() % 16 == 4
        _, c = plan.process(src[1:], out=dst[1:-1])
        assert c == counts[i] and same(host(dst[1:-1]).reshape(T, -1), rows[i])
        assert host(dst)[0] == 7.0 and host(dst)[-1] == 7.0                  # nothing outside the rows is written
    plan.close()


@pytest.mark.parametrize("shape", [(160, 147, None, 3, 7, 23), (147, 160, None, 65, 100, 10)], ids=ident)
def test_reset_gives_a_new_plan(gab, shape):
    xs, rows, counts, _, _ = case(shape)
    plan = make(gab, shape)
    run(plan, xs[:3])
    assert host(plan.state()[0]).any() and plan.state()[1] == 3 % plan.period
    plan.reset()
    h, k = plan.state()
    assert not host(h).view(np.uint32).any() and k == 0
    got, got_counts = run(plan, xs[:4])
    assert got_counts == counts[:4] and same(got, rows[:4])
    plan.close()


@pytest.mark.parametrize("shape", [(160, 147, None, 65, 64, 4), (3, 2, 6, 3, 100, 4), (2, 5, 16, 66, 100, 5),
                                   (3, 200, 8, 3, 64, 12)], ids=ident)
def test_set_taps_mid_stream_one_hot_selects_exactly(gab, shape):
    """After two buffers the table becomes one-hot, row p at j = (3 p) mod K: every later output is the input sample
    w[i - j] itself, i and p from exact integers here, no restatement involved; history and position were kept."""
    up, down, K, T, B, n = shape
    xs, rows, counts, _, _ = case(shape)
    plan = make(gab, shape)
    L, M, K = plan.up, plan.down, plan.ntaps
    got, _ = run(plan, xs[:2])
    assert same(got, rows[:2])
    sel = (3 * np.arange(L)) % K
    taps = np.zeros((L, K), F32)
    taps[np.arange(L), sel] = 1.0
    plan.set_taps(dev(taps))
    assert same(host(plan.taps()), taps)
    stream = np.concatenate(list(xs), axis=1)                                 # [T][n B]
    m = -(-(2 * B * L) // M)                                                  # the first output of buffer 2
    for k in (2, 3):
        out, c = plan.process(dev(xs[k].reshape(-1)))
        assert c == counts[k]
        idx = np.arange(m, m + c)
        src = (idx * M) // L - sel[(idx * M) % L]
        want = np.where(src[None, :] >= 0, stream[:, np.maximum(src, 0)], F32(0))
        got = host(out)[:, :c]
        clean = slice(0, T - 1)                                               # the last track holds the NaN and the infinity
        assert np.array_equal(bits(got[clean]), bits(want[clean]))
        assert not host(out)[:, c:].any()
        m += c
    plan.close()


def test_refusals_leave_the_plan_as_it_was(gab):
    import ctypes as C
    shape = (160, 147, None, 65, 64, 4)
    up, down, K, T, B, n = shape
    xs, rows, counts, _, _ = case(shape)
    plan = make(gab, shape)
    got, _ = run(plan, xs[:1])
    assert same(got, rows[:1])
    bad = resample_taps32(up, down, plan.ntaps).copy()
    bad[5, 9] = np.inf
    bad[17, 2] = np.nan                                                       # the first in index order is named
    with pytest.raises(gab.GabError) as e:
        plan.set_taps(dev(bad))
    assert "phase 5 tap 9" in str(e.value) and e.value.code == -1
    lib = gab.lib
    x1 = dev(xs[1].reshape(-1))
    out = dev(np.zeros((T, plan.out_capacity), F32))
    cnt = (C.c_int * 1)()
    st = C.c_void_p(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
    assert lib.gab_resample_process_batch(plan._h, ptr(x1), ptr(out), 0, cnt, st) == -1
    assert b"n_buffers" in lib.gab_last_error()
    assert lib.gab_resample_process(plan._h, None, ptr(out), cnt, st) == -1
    assert lib.gab_resample_process(plan._h, ptr(x1), ptr(out), None, st) == -1
    assert lib.gab_resample_set_taps(plan._h, None, st) == -1
    for args, code in (((T, B, 0, 147, 32), -1), ((T, B, 160, 147, 31), -1), ((T, B, 1023, 1024, 32), -3)):
        with pytest.raises(gab.GabError) as e:
            gab.ResamplePlan(*args)
        assert e.value.code == code
    assert same(host(plan.taps()), resample_taps32(up, down, plan.ntaps)) and plan.state()[1] == 1
    got, got_counts = run(plan, xs[1:])
    assert got_counts == counts[1:] and same(got, rows[1:])
    plan.close()
