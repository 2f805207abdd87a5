"""The crossover plan on the device, held bit for bit against tests/test_crossover_host.py's Twin: the bands AND the whole
state array, for every launch form, alignment, track count and band count; sets, refusals, reset, shards, the edges of
float32, captured graphs, the multiband strip (CrossoverPlan -> DynamicsPlan -> MixPlan) and, as the one check that does
not go through a twin written by the same hand, EqPlan cascades of scipy's Butterworth sections.

The twin runs ONE stream of 1536 samples on 130 tracks per band count (reference()); a case (T, B, K) is the first T
tracks and the first 3 B samples of it, which a recurrence per track and sample allows.  Every test here fails on a
commit without gab_xover_*."""
import ctypes
import functools

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_crossover_host import Twin, noise, rows32, xover_first_refused

pytestmark = pytest.mark.gpu

TRACKS = [1, 63, 65, 130]                 # below a wave's tracks for every K (16, 32, 64), across them, two and more groups
BUFSIZES = [1, 63, 64, 65, 200, 512]      # the chunk edge, a multiple of 4 that is no chunk, eight chunks
BANDS = [2, 3, 4]
N_BUFFERS = 3
MAX_T, MAX_B = max(TRACKS), max(BUFSIZES)


def same(a, b):
    """Bit for bit; two NaNs count as the same."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def splits(T, K, seed):
    """[T][S][3]: every track its own ascending splits, split j within the j-th of S equal parts (in octaves) of
    20 Hz .. 20 kHz."""
    S = K - 1
    edges = np.geomspace(20.0, 20000.0, S + 1)
    u = np.random.RandomState(seed).uniform(0.02, 0.98, (T, S))
    f = edges[:-1] * (edges[1:] / edges[:-1]) ** u
    return np.stack([rows32(row) for row in f])


@functools.lru_cache(maxsize=None)
def reference(K):
    """(rows, x [130][1536], bands [K][130][1536], {n: the state behind n samples}), read only."""
    rows, x = splits(MAX_T, K, 100 + K), noise(MAX_T, N_BUFFERS * MAX_B, 200 + K)
    twin = Twin(MAX_T, MAX_B, K)
    twin.set_splits(rows)
    marks = sorted({k * B for B in BUFSIZES for k in range(1, N_BUFFERS + 1)})
    out, states, at = [], {}, 0
    for m in marks:
        out.append(twin.process(x[:, at:m]))
        states[m] = twin.state.copy()
        at = m
    bands = np.concatenate(out, axis=2)
    for a in (rows, x, bands, *states.values()):
        a.setflags(write=False)
    return rows, x, bands, states


def run(plan, x, out=None):
    """x [T][B] -> [K][T][B] on the host."""
    y = plan.process(dev(np.ascontiguousarray(x).ravel()), out=out)
    return host(y).reshape(plan.bands, plan.tracks, plan.bufsize)


def small(T, B, K, n, seed):
    """A stream of its own: (rows, xs [n][T][B], ys [n][K][T][B], states [n], twin)."""
    rows, xs = splits(T, K, seed), noise(T, n * B, seed + 1).reshape(T, n, B).transpose(1, 0, 2)
    twin = Twin(T, B, K)
    twin.set_splits(rows)
    ys, states = [], []
    for k in range(n):
        ys.append(twin.process(xs[k]))
        states.append(twin.state.copy())
    return rows, xs, np.stack(ys), states, twin


# ---- 1. the contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", BANDS)
@pytest.mark.parametrize("B", BUFSIZES)
@pytest.mark.parametrize("T", TRACKS)
def test_contract_bit_for_bit(gab, T, B, K):
    rows, x, bands, states = reference(K)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows[:T]))
    assert same(host(plan.splits()), rows[:T])
    for k in range(N_BUFFERS):
        y = run(plan, x[:T, k * B:(k + 1) * B])
        assert same(y, bands[:, :T, k * B:(k + 1) * B]), k
        assert same(host(plan.state()), states[(k + 1) * B][:T]), k
    plan.close()


# ---- 2. launch forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,K", [(70, 100, 2), (70, 100, 3), (70, 100, 4), (33, 65, 4)])
def test_batch_of_three_is_three_single_launches(gab, T, B, K):
    rows, xs, ys, states, _ = small(T, B, K, 3, 300 + K)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows))
    y = host(plan.process_batch(dev(xs.ravel()))).reshape(3, K, T, B)
    assert same(y, ys) and same(host(plan.state()), states[2])
    plan.close()


def test_mixed_calls_are_the_per_buffer_stream(gab):
    T, B, K = 37, 72, 4
    rows, xs, ys, states, _ = small(T, B, K, 6, 310)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows))
    assert same(run(plan, xs[0]), ys[0])
    assert same(host(plan.process_batch(dev(xs[1:3].ravel()))).reshape(2, K, T, B), ys[1:3])
    assert same(run(plan, xs[3]), ys[3])
    assert same(host(plan.process_batch(dev(xs[4:6].ravel()))).reshape(2, K, T, B), ys[4:6])
    assert same(host(plan.state()), states[5])
    plan.close()


@pytest.mark.parametrize("K", BANDS)
def test_pointers_four_bytes_off_give_the_same_bits(gab, K):
    import torch
    T, B = 35, 64                                                      # B % 4 == 0: alignment alone picks the form
    rows, xs, ys, states, _ = small(T, B, K, 2, 320 + K)
    for off_in, off_out in ((1, 0), (0, 1), (1, 1), (3, 2)):
        plan = gab.CrossoverPlan(T, B, K)
        plan.set_splits(dev(rows))
        x = torch.zeros(T * B + 4, device="cuda")[off_in:off_in + T * B]
        out = torch.zeros(K * T * B + 4, device="cuda")[off_out:off_out + K * T * B]
        assert (x.data_ptr() % 16 != 0) == (off_in != 0) and (out.data_ptr() % 16 != 0) == (off_out != 0)
        for k in range(2):
            x.copy_(dev(xs[k].ravel()))
            plan.process(x, out=out)
            assert same(host(out).reshape(K, T, B), ys[k]), (off_in, off_out, k)
        assert same(host(plan.state()), states[1])
        plan.close()


# ---- 3. sets --------------------------------------------------------------------------------------------------------
def test_set_splits_tracks_mid_stream(gab):
    T, B, K = 65, 64, 3
    rows, xs4, ys_unmoved, states, _ = small(T, B, K, 4, 330)          # four buffers with no set
    plan, twin = gab.CrossoverPlan(T, B, K), Twin(T, B, K)
    plan.set_splits(dev(rows))
    twin.set_splits(rows)
    for k in range(2):
        assert same(run(plan, xs4[k]), twin.process(xs4[k])), k
    moved = splits(5, K, 332)
    plan.set_splits(dev(moved), first_track=3, n_tracks=5)
    twin.set_splits(moved, first_track=3)
    assert same(host(plan.state()), states[1])                         # a set keeps the state
    assert same(host(plan.splits()), twin.rows)
    others = np.r_[0:3, 8:T]
    for k in range(2, 4):
        y, want = run(plan, xs4[k]), twin.process(xs4[k])
        assert same(y, want) and same(host(plan.state()), twin.state), k
        assert same(y[:, others], ys_unmoved[k][:, others]), k         # no other track's bits move
        assert not same(y[:, 3:8], ys_unmoved[k][:, 3:8]), k           # and the set acts from the next buffer
    plan.close()


def test_a_refused_table_changes_nothing(gab):
    T, B, K = 20, 64, 3
    rows, xs, ys, states, _ = small(T, B, K, 3, 340)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows))
    assert same(run(plan, xs[0]), ys[0])
    good = splits(T, K, 341)
    tiny = np.float32(-1e-30)

    def swapped_ratio(r):                                              # the sum kept, the ratio spoilt
        d = np.float32(1e-3) * r[1]
        return np.array([r[0], r[1] + d, r[2] - np.float32(np.sqrt(2.0)) * d], np.float32)

    # (track, split, field or None for the whole row, value, the field of the track's 3 S values that is named)
    cases = [(4, 0, 0, np.nan, 0), (5, 1, 1, np.inf, 4), (6, 0, 2, -np.inf, 2),             # not finite
             (7, 1, 0, 0.0, 3), (8, 0, 0, 1.5, 0), (9, 0, 0, tiny, 0),                       # a1 outside (0, 1]
             (10, 1, 1, tiny, 4), (11, 0, 1, 1.0, 1),                                        # a2 outside [0, 1)
             (12, 1, 2, tiny, 5), (13, 0, 2, 1.0, 2),                                        # a3 outside [0, 1)
             (14, 1, 0, good[14, 1, 0] * np.float32(0.999), 5),                              # the sum
             (15, 1, None, swapped_ratio(good[15, 1]), 5)]                                   # the ratio
    for t, s, f, value, named in cases:
        bad = good.copy()
        if f is None:
            bad[t, s] = value
            assert abs((bad[t, s, 0] + np.float32(np.sqrt(2.0)) * bad[t, s, 1] + bad[t, s, 2]) - 1.0) < 2.0 ** -21
        else:
            bad[t, s, f] = value
        bad[t + 1, 0, 0] = np.nan                                      # the FIRST offender is named
        assert xover_first_refused(bad) == t * 3 * (K - 1) + named     # the host twin of the rule agrees
        with pytest.raises(gab.GabError) as e:
            plan.set_splits(dev(bad))
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
        assert "track %d field %d " % (t, named) in str(e.value), str(e.value)
    bad = good[:4].copy()
    bad[2, 1, 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_splits(dev(bad), first_track=3)
    assert "track 5 field 4 " in str(e.value)
    assert same(host(plan.splits()), rows) and same(host(plan.state()), states[0])
    for k in (1, 2):
        assert same(run(plan, xs[k]), ys[k]), k
    plan.close()


def test_process_before_any_set_is_refused(gab):
    plan = gab.CrossoverPlan(4, 64, 3)
    x = dev(noise(4, 64, 1).ravel())
    for call in (lambda: plan.process(x), lambda: plan.process_batch(x)):
        with pytest.raises(gab.GabError) as e:
            call()
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG and "no splits have been set" in str(e.value)
    with pytest.raises(gab.GabError):                                  # a refused set is no set
        plan.set_splits(dev(np.zeros((4, 2, 3), np.float32)))
    with pytest.raises(gab.GabError):
        plan.process(x)
    rows = splits(4, 3, 2)
    plan.set_splits(dev(rows))
    twin = Twin(4, 64, 3)
    twin.set_splits(rows)
    assert same(run(plan, host(x).reshape(4, 64)), twin.process(host(x).reshape(4, 64)))
    plan.close()


# ---- 4. reset and shards --------------------------------------------------------------------------------------------
def test_reset_zeroes_the_state_and_keeps_the_rows(gab):
    T, B, K = 18, 70, 4
    rows, xs, ys, states, _ = small(T, B, K, 2, 350)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows))
    for k in range(2):
        assert same(run(plan, xs[k]), ys[k])
    assert host(plan.state()).any()
    plan.reset()
    assert not bits(host(plan.state())).any() and same(host(plan.splits()), rows)
    for k in range(2):                                                 # the stream again, from the start
        assert same(run(plan, xs[k]), ys[k]) and same(host(plan.state()), states[k]), k
    plan.close()


@pytest.mark.parametrize("K", BANDS)
def test_a_shard_is_those_rows_of_the_whole(gab, K):
    rows, x, bands, states = reference(K)
    lo, hi, B = 64, 130, 200
    shard = gab.CrossoverPlan(hi - lo, B, K)
    shard.set_splits(dev(rows[lo:hi]))
    for k in range(N_BUFFERS):
        y = run(shard, x[lo:hi, k * B:(k + 1) * B])
        assert same(y, bands[:, lo:hi, k * B:(k + 1) * B]) and same(host(shard.state()), states[(k + 1) * B][lo:hi]), k
    shard.close()


# ---- 5. where float32 ends ------------------------------------------------------------------------------------------
def test_a_tail_dies_through_the_subnormals(gab):
    """An impulse of 2^-100, then silence: the tail runs down through the subnormals with the twin's bits, so nothing is
    flushed to zero on the way.  Where it ends: the issue expected +-0 in every state.  The contract's own arithmetic
    does not do that: with round-to-nearest a section stops moving once a2 v3 and a3 v3 round to nothing against its
    states, which leaves states of a few units of 2^-149 behind (Twin on 200 random tracks of splits between 2 and 23
    kHz: 2 of 200 reach +-0 for K = 2, none for K = 3 and 4; the largest state 16, 18 and 20 units).  What is held here
    instead: the bits of the twin all the way, a rest of at most 64 units of 2^-149 for these splits (g >= 0.34, a3 >=
    0.07: |v3| below 1 / (2 a3) = 7 units moves nothing, and the four sections of a band's chain add up) over the last
    four buffers: it wanders there (the twin: 10, 12, 10, 8, 8 units behind buffers 1 to 5) and does not grow."""
    T, B, K, n = 3, 64, 4, 6
    rows = np.stack([rows32(f) for f in ([6000.0, 9000.0, 14000.0], [5000.0, 11000.0, 20000.0], [8000.0, 8100.0, 12000.0])])
    plan, twin = gab.CrossoverPlan(T, B, K), Twin(T, B, K)
    plan.set_splits(dev(rows))
    twin.set_splits(rows)
    x = np.zeros((T, B), np.float32)
    x[:, 0] = 2.0 ** -100
    tiny, rests = False, []
    for k in range(n):
        y, want = run(plan, x), twin.process(x)
        assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(host(plan.state())), bits(twin.state)), k
        tiny |= bool(((np.abs(want) > 0) & (np.abs(want) < 2.0 ** -126)).any())
        rests.append(host(plan.state()))
        x[:, 0] = 0.0
    assert tiny                                                        # the tail was subnormal on its way
    print("\nthe tail rests at %g units of 2^-149" % (np.abs(rests[-1]).max() / 2.0 ** -149))
    assert all(np.abs(r).max() <= 64 * 2.0 ** -149 for r in rests[2:])
    plan.close()


def test_signed_zeros(gab):
    T, B, K = 5, 70, 3
    rows = splits(T, K, 360)
    for z in (np.float32(0.0), np.float32(-0.0)):
        plan, twin = gab.CrossoverPlan(T, B, K), Twin(T, B, K)
        plan.set_splits(dev(rows))
        twin.set_splits(rows)
        x = np.full((T, B), z, np.float32)
        for k in range(2):
            y, want = run(plan, x), twin.process(x)
            assert np.array_equal(bits(y), bits(want)) and np.array_equal(bits(host(plan.state())), bits(twin.state)), k
            assert not y.any()
        plan.close()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_what_is_not_finite_stays_in_its_track(gab, value):
    T, B, K = 5, 70, 4
    rows, xs, ys, states, _ = small(T, B, K, 3, 370)
    plan, twin = gab.CrossoverPlan(T, B, K), Twin(T, B, K)
    plan.set_splits(dev(rows))
    twin.set_splits(rows)
    others = [0, 1, 3, 4]
    for k in range(3):
        x = xs[k].copy()
        if k == 0:
            x[2, 10] = value
        y, want = run(plan, x), twin.process(x)
        assert same(y, want) and same(host(plan.state()), twin.state), k
        # in every band of track 2 from that sample on, the next buffers included
        assert not np.isfinite(y[:, 2, 10 if k == 0 else 0:]).any(), k
        assert np.isfinite(y[:, 2, :10]).all() or k > 0
        # and in no bit of another track
        assert same(y[:, others], ys[k][:, others]) and same(host(plan.state())[others], states[k][others]), k
    plan.reset()
    twin.reset()
    for k in range(2):                                                 # after reset track 2 is clean
        assert same(run(plan, xs[k]), ys[k]) and same(host(plan.state()), states[k]), k
    plan.close()


# ---- 6. captured graphs ---------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_bits_of_plain_calls(gab):
    import torch
    T, B, K = 70, 100, 4
    rows, xs, ys, states, _ = small(T, B, K, 4, 380)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows))
    assert same(run(plan, xs[0]), ys[0])
    x, out = torch.zeros(T * B, device="cuda"), torch.zeros(K * T * B, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(x, out)
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same(host(plan.state()), states[0])                         # the capture recorded a launch without running it
    for k in range(1, 4):
        x.copy_(dev(xs[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same(host(out).reshape(K, T, B), ys[k]) and same(host(plan.state()), states[k]), k
    del graph
    plan.close()


# ---- 7. the multiband strip -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("captured", [False, True])
def test_the_multiband_strip_is_the_composed_restatement(gab, captured):
    """CrossoverPlan(K = 3) -> DynamicsPlan on the 3 T tracks of the band block, in place -> MixPlan, 3 T tracks to T buses
    with unit gains on a track's own three bands: a multiband compressor, on one stream with no host wait between."""
    import torch
    from test_dynamics_host import Twin as DynTwin, dyn_mix
    from test_mix_host import Twin as MixTwin
    T, B, K, n = 5, 64, 3, 4
    rows, xs, ys, states, xtwin = small(T, B, K, n, 390)
    pd = dyn_mix(K * T, 1)
    gains = np.zeros((K * T, T), np.float32)
    for b in range(K):
        gains[b * T + np.arange(T), np.arange(T)] = 1.0
    xo, dyn, mix = gab.CrossoverPlan(T, B, K), gab.DynamicsPlan(K * T, B), gab.MixPlan(K * T, B, T)
    dtwin, mtwin = DynTwin(K * T, B), MixTwin(K * T, B, T, *mix.form)
    xo.set_splits(dev(rows))
    dyn.set_params(dev(pd), ramp=False)
    dtwin.set_params(pd, ramp=False)
    mix.set_gains(dev(gains), ramp=False)
    mtwin.set_gains(gains, ramp=False)
    want = [mtwin.process(dtwin.process(ys[k].reshape(K * T, B))[0]) for k in range(n)]
    x, block, bus = torch.zeros(T * B, device="cuda"), torch.zeros(K * T * B, device="cuda"), torch.zeros(T * B, device="cuda")
    if captured:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            xa, da, ma = xo.prepare(x, block), dyn.prepare(block, block), mix.prepare(block, bus)
            with torch.cuda.graph(graph, stream=side):
                xo.launch(xa)
                dyn.launch(da)
                mix.launch(ma)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    for k in range(n):
        x.copy_(dev(xs[k].ravel()))
        if captured:
            graph.replay()
        else:
            xo.process(x, out=block)
            dyn.process(block, out=block)
            mix.process(block, out=bus)
        torch.cuda.synchronize()
        assert same(host(bus).reshape(T, B), want[k]), k
    assert same(host(xo.state()), states[n - 1]) and same(host(dyn.state()), dtwin.s)
    assert same(host(mix.gains()[0]), mtwin.cur)
    if captured:
        del graph
    for p in (xo, dyn, mix):
        p.close()


# ---- 8. bad arguments, memory ---------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, K = 20, 64, 3
    rows, xs, ys, states, _ = small(T, B, K, 2, 400)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 2), (4, 0, 2), (4, 64, 1), (4, 64, 5)):
        assert lib.gab_xover_create(ctypes.byref(h), *args) == bad and not h.value, args
    for bands in (1, 5):
        with pytest.raises(gab.GabError):
            gab.CrossoverPlan(4, 64, bands)
    plan = gab.CrossoverPlan(T, B, K)
    plan.set_splits(dev(rows))
    assert same(run(plan, xs[0]), ys[0])
    hp = plan._h
    big = dev(np.zeros((K + 1) * T * B, np.float32))
    buf, rd = dev(xs[1].ravel()), dev(rows)
    q, o, rp = (ctypes.c_void_p(t.data_ptr()) for t in (buf, big, rd))
    assert lib.gab_xover_process(hp, None, o, None) == bad and lib.gab_xover_process(hp, q, None, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_xover_process_batch(hp, q, o, 0, None) == bad and lib.gab_xover_process_batch(hp, q, o, -2, None) == bad
    assert b"n_buffers" in lib.gab_last_error()
    # d_out on d_in, d_out ending on d_in's first word, d_in on d_out's last word
    at = lambda words: ctypes.c_void_p(big.data_ptr() + 4 * words)     # noqa: E731
    for d_in, d_out in ((at(0), at(0)), (at(K * T * B - 1), at(0)), (at(0), at(T * B - 1))):
        assert lib.gab_xover_process(hp, d_in, d_out, None) == bad and b"overlap" in lib.gab_last_error()
    assert lib.gab_xover_set_splits(hp, None, None) == bad and lib.gab_xover_set_splits(None, rp, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_xover_set_splits_tracks(hp, rp, first, n, None) == bad, (first, n)
        assert b"outside the plan" in lib.gab_last_error()
    assert lib.gab_xover_splits(hp, None, None) == bad and lib.gab_xover_state(hp, None, None) == bad
    with pytest.raises(ValueError):
        plan.set_splits(dev(rows.ravel()[:5]))
    with pytest.raises(ValueError):
        plan.set_splits(dev(rows[:3]))
    # the input right in front of the band block is no overlap
    assert lib.gab_xover_process(hp, at(0), at(T * B), None) == 0
    big[:T * B].copy_(buf)
    plan.reset()
    for k in range(2):
        assert same(run(plan, xs[k]), ys[k]) and same(host(plan.state()), states[k]), k
    plan.close()


def test_fifty_plans_leave_free_device_memory_where_it_was(gab):
    import torch
    T, B, K = 16384, 128, 4                                            # 0.6 MiB of rows and 1.5 MiB of state per plan
    x = dev(noise(1, T * B, 9).ravel())
    out = torch.empty(K * T * B, device="cuda")
    rows = dev(np.tile(rows32([200.0, 2000.0, 8000.0]), (T, 1, 1)))

    def cycle():
        plan = gab.CrossoverPlan(T, B, K)
        plan.set_splits(rows)
        plan.process(x, out=out)
        plan.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(50):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) <= 2 * 1024 * 1024, (free0, free1)


# ---- 9. against what exists -----------------------------------------------------------------------------------------
def test_the_outer_bands_agree_with_eq_cascades_of_butterworth_sections(gab):
    """Band 0 and band K - 1 of a split at 1 kHz are a second-order Butterworth low-pass, and high-pass, twice.  EqPlan's
    ordered form on scipy's sections is another arithmetic (6e-6 of float64 here), so this is no bit yardstick; it
    catches a wrong topology or a swapped output, which a twin written by the same hand would share."""
    from scipy import signal
    T, B, n = 4, 512, 4
    x = noise(T, n * B, 410).reshape(T, n, B).transpose(1, 0, 2)
    plan = gab.CrossoverPlan(T, B, 2)
    plan.set_splits(dev(np.tile(gab.crossover_rows(1000.0), (T, 1, 1))))
    eqs = []
    for kind in ("lowpass", "highpass"):
        sos = signal.butter(2, 1000.0, kind, fs=48000.0, output="sos")
        eq = gab.EqPlan(T, B, 2)
        eq.set_sos(np.concatenate([sos, sos]))
        eqs.append(eq)
    worst = 0.0
    for k in range(n):
        xd = dev(x[k].ravel())
        y = host(plan.process(xd)).reshape(2, T, B)
        for band, eq in enumerate(eqs):
            want = host(eq.process(xd, sequential=True)).reshape(T, B)
            err = np.abs(y[band].astype(np.float64) - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err < 1e-4, (k, band, err)
    print("\nbands of a 1 kHz split against EqPlan's Butterworth cascades: %.2e of peak" % worst)
    plan.close()
    for eq in eqs:
        eq.close()
