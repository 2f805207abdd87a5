"""The saturator plan on the device, held bit for bit to tests/saturator_twin.py and to the composition it restates:
ResamplePlan (up R) -> SaturatorPlan.apply -> ResamplePlan (down R), outputs and both histories."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import saturator_twin as st
from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from saturator_twin import F32, SatTwin

pytestmark = pytest.mark.gpu

TRACKS, BUFSIZES, RATIOS = (1, 3, 65, 130), (1, 5, 64, 100, 512), (1, 2, 4, 8)
PAIRS = ("small", "mid", "default")                 # (Ku, Kd) = (4, 2R), (6, 4R), (32, 32R)


def taps_of(pair, R):
    return (0, 0) if R == 1 else {"small": (4, 2 * R), "mid": (6, 4 * R), "default": (32, 32 * R)}[pair]


#          T    B    R  pair       curve
CENSUS = [(1, 1, 2, "small", "hard"),
          (3, 5, 4, "default", "cubic"),            # B < Ku - 1 and R B < Kd - 1
          (65, 64, 8, "mid", "rational"),
          (130, 100, 2, "mid", "cubic"),
          (3, 512, 4, "default", "hard"),
          (130, 512, 1, "small", "rational"),
          (65, 5, 2, "mid", "hard"),                # B = Ku - 1: neither history is longer than a buffer
          (3, 1, 8, "default", "rational"),
          (130, 64, 4, "small", "cubic"),
          (1, 100, 8, "default", "hard"),
          (65, 512, 2, "default", "cubic"),
          (3, 64, 1, "mid", "hard"),
          (1, 5, 1, "default", "cubic")]
N_CALLS = 6


def short_class(B, R, pair):
    Ku, Kd = taps_of(pair, R)
    return (B < Ku - 1, R * B < Kd - 1)


def test_the_census_reaches_every_class():
    for values, column in ((TRACKS, 0), (BUFSIZES, 1), (RATIOS, 2), (PAIRS, 3), (st.CURVES, 4)):
        assert {c[column] for c in CENSUS} == set(values), column
    possible = {short_class(B, R, pair) for B, R, pair in itertools.product(BUFSIZES, (2, 4, 8), PAIRS)}
    assert {short_class(B, R, pair) for _, B, R, pair, _ in CENSUS if R > 1} == possible and len(possible) >= 2
    assert any(B % 4 for _, B, _, _, _ in CENSUS) and any(B % 4 == 0 for _, B, _, _, _ in CENSUS)   # both load widths
    assert any(T > 16 and T % 16 for T, _, _, _, _ in CENSUS)             # more than a workgroup, the last one partial


def same(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rows_mix(T, seed):
    """A table [T][3]: drives that reach the rails and drives that do not, biases of both signs."""
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(0.5, 6.0, T), rng.uniform(-0.5, 0.5, T), rng.uniform(0.25, 2.0, T)], axis=1).astype(F32)


def signal(n, T, B, seed):
    return (np.random.RandomState(seed).uniform(-1.0, 1.0, (n, T, B)) * 1.25).astype(F32)


def make(gab, case, rows=None):
    T, B, R, pair, curve = case
    Ku, Kd = taps_of(pair, R)
    plan = gab.SaturatorPlan(T, B, R, curve, Ku or None, Kd or None)
    assert (plan.oversample, plan.up_taps, plan.down_taps, plan.latency) == (R, Ku, Kd, st.latency(R, Ku, Kd))
    if rows is not None:
        plan.set_params(dev(rows), ramp=False)
    return plan


def twin_of(case, rows=None):
    T, B, R, pair, curve = case
    Ku, Kd = taps_of(pair, R)
    twin = SatTwin(T, B, R, curve, Ku or None, Kd or None)
    if rows is not None:
        twin.set_params(rows, ramp=False)
    return twin


def same_state(plan, twin):
    if twin.R == 1:
        return plan.state() == (None, None)
    a, b = plan.state()
    return same(host(a), twin.hist_in) and same(host(b), twin.hist_os)


@functools.lru_cache(maxsize=None)
def reference(case, ramp_at=2):
    """Six buffers through the twin, rows p0 at once and p1 ramped in over buffer `ramp_at`: (p0, p1, xs, ys, hists)."""
    T, B = case[:2]
    p0, p1, xs = rows_mix(T, 1), rows_mix(T, 2), signal(N_CALLS, T, B, 3)
    twin = twin_of(case, p0)
    ys, hists = [], []
    for i in range(N_CALLS):
        if i == ramp_at:
            twin.set_params(p1, ramp=True)
        ys.append(twin.process(xs[i]))
        hists.append(None if twin.R == 1 else (twin.hist_in.copy(), twin.hist_os.copy()))
    for a in (p0, p1, xs):
        a.setflags(write=False)
    return p0, p1, xs, ys, hists


def same_hist(plan, hist):
    if hist is None:
        return plan.state() == (None, None)
    return all(same(host(a), b) for a, b in zip(plan.state(), hist))


SMALL, ODD, WIDE = CENSUS[1], CENSUS[6], CENSUS[3]


# ---- 1. the contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CENSUS)
def test_fused_against_the_twin_after_every_call(gab, case):
    p0, p1, xs, ys, hists = reference(case)
    plan = make(gab, case, p0)
    for i in range(N_CALLS):
        if i == 2:
            plan.set_params(dev(p1))
        y = host(plan.process(dev(xs[i].ravel()))).reshape(xs[i].shape)
        assert same(y, ys[i]), i
        assert same_hist(plan, hists[i]), i
    cur, tgt = plan.params()
    assert same(host(cur), p1) and same(host(tgt), p1)
    plan.close()


@pytest.mark.parametrize("case", CENSUS)
def test_fused_against_the_composition_on_the_device(gab, case):
    """ResamplePlan up -> apply -> ResamplePlan down, steady and with a ramp pending; histories included."""
    T, B, R, pair, curve = case
    Ku, Kd = taps_of(pair, R)
    p0, p1, xs = rows_mix(T, 4), rows_mix(T, 5), signal(4, T, B, 6)
    fused, shaper = make(gab, case, p0), make(gab, case, p0)
    up = gab.ResamplePlan(T, B, R, 1, Ku) if R > 1 else None
    down = gab.ResamplePlan(T, R * B, 1, R, Kd) if R > 1 else None
    for i in range(4):
        if i == 1:
            fused.set_params(dev(p1))
            shaper.set_params(dev(p1))
        x = dev(xs[i].ravel())
        y = fused.process(x)
        if R == 1:
            want = shaper.apply(x)
        else:
            u, n = up.process(x)
            assert n == R * B
            v = shaper.apply(u.view(-1))
            want, n = down.process(v)
            assert n == B
            hin, hos = fused.state()
            assert same(host(hin), host(up.state()[0])) and same(host(hos), host(down.state()[0])), i
        assert same(host(y).reshape(T, B), host(want).reshape(T, B)), i
    for p in (fused, shaper, up, down):
        if p:
            p.close()


@pytest.mark.parametrize("case", [SMALL, ODD, WIDE, CENSUS[5], CENSUS[2]])
def test_apply_against_the_twins_curve_stage_in_place_and_apart(gab, case):
    T, B, R, pair, curve = case
    p0, p1 = rows_mix(T, 7), rows_mix(T, 8)
    us = signal(3, T, R * B, 9) * F32(2.0)
    plan, twin = make(gab, case, p0), twin_of(case, p0)
    got = host(plan.apply(dev(us[0].ravel()))).reshape(1, T, R * B)                  # apart, steady
    assert same(got, twin.apply(us[:1]))
    plan.set_params(dev(p1))
    twin.set_params(p1, ramp=True)
    want = twin.apply(us)                                                             # three blocks, the first ramps
    buf = dev(us.ravel())
    assert plan.apply(buf, out=buf) is buf                                            # in place
    assert same(host(buf).reshape(3, T, R * B), want)
    import torch
    big = torch.zeros(3 * T * R * B + 2, device="cuda")                               # 4 bytes off alignment, steady
    big[1:-1] = dev(us.ravel())
    plan.apply(big[1:-1], out=big[1:-1])
    assert same(host(big)[1:-1].reshape(3, T, R * B), twin.apply(us))
    assert same_state(plan, twin)                                                     # no history moved
    plan.close()


# ---- 2. the launch forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CENSUS)
def test_batch_is_its_single_calls(gab, case):
    p0, p1, xs, ys, hists = reference(case)
    plan = make(gab, case, p0)
    T, B = case[:2]
    got = host(plan.process_batch(dev(xs[:2].ravel()))).reshape(2, T, B)
    assert same(got, np.stack(ys[:2])) and same_hist(plan, hists[1])
    plan.set_params(dev(p1))                                                          # only the first buffer ramps
    got = host(plan.process_batch(dev(xs[2:].ravel()))).reshape(N_CALLS - 2, T, B)
    assert same(got, np.stack(ys[2:])) and same_hist(plan, hists[-1])
    plan.close()


@pytest.mark.parametrize("case", [SMALL, ODD, WIDE, CENSUS[4], CENSUS[8]])
def test_four_bytes_off_alignment(gab, case):
    import torch
    p0, p1, xs, ys, hists = reference(case)
    T, B = case[:2]
    plan = make(gab, case, p0)
    big, out = torch.zeros(T * B + 1, device="cuda"), torch.zeros(T * B + 1, device="cuda")
    for i in range(N_CALLS):
        if i == 2:
            plan.set_params(dev(p1))
        big[1:] = dev(xs[i].ravel())
        plan.process(big[1:], out=out[1:])
        assert same(host(out)[1:].reshape(T, B), ys[i]) and same_hist(plan, hists[i]), i
    plan.close()


@pytest.mark.parametrize("case", [WIDE, CENSUS[2]])
def test_a_shard_of_tracks_is_those_tracks_of_the_whole(gab, case):
    p0, p1, xs, ys, hists = reference(case)
    T, B, R, pair, curve = case
    lo, hi = 17, 50
    shard = make(gab, (hi - lo, B, R, pair, curve), p0[lo:hi])
    for i in range(N_CALLS):
        if i == 2:
            shard.set_params(dev(p1[lo:hi]))
        y = host(shard.process(dev(xs[i][lo:hi].ravel()))).reshape(hi - lo, B)
        assert same(y, ys[i][lo:hi]), i
    assert all(same(host(a), b[lo:hi]) for a, b in zip(shard.state(), hists[-1]))
    shard.close()


def test_reset_gives_a_new_plans_bits_and_drops_a_ramp(gab):
    for case in (SMALL, WIDE):
        p0, p1, xs, ys, hists = reference(case, ramp_at=None)
        T, B = case[:2]
        plan = make(gab, case, p0)
        plan.process(dev(xs[3].ravel()))
        plan.set_params(dev(p0))                                 # a ramp (to the same rows) is pending: reset drops it
        plan.reset()
        assert all(not host(a).any() for a in plan.state())
        for i in range(3):
            assert same(host(plan.process(dev(xs[i].ravel()))).reshape(T, B), ys[i]), i
        plan.close()


def test_rows_taps_and_a_ranged_set_mid_stream(gab):
    case = WIDE
    T, B, R, pair, curve = case
    Ku, Kd = taps_of(pair, R)
    p0, p1, xs = rows_mix(T, 10), rows_mix(T, 11), signal(N_CALLS, T, B, 12)
    rng = np.random.RandomState(13)
    up2, down2 = rng.uniform(-0.5, 0.5, (R, Ku)).astype(F32), rng.uniform(-0.3, 0.3, (1, Kd)).astype(F32)
    plan, twin = make(gab, case, p0), twin_of(case, p0)
    u0, d0 = plan.taps()
    assert same(host(u0), twin.up.taps) and same(host(d0).reshape(1, -1), twin.down.taps)   # the one design function
    for i in range(N_CALLS):
        if i == 1:                                               # rows 20..59 ramped, the others stay
            plan.set_params(dev(p1[20:60]), ramp=True, first_track=20)
            twin.set_params(p1[20:60], ramp=True, first_track=20)
        if i == 3:                                               # new taps: in force from this buffer, histories kept
            plan.set_taps(dev(up2), dev(down2.ravel()))
            twin.set_taps(up2, down2)
        if i == 4:                                               # rows at once
            plan.set_params(dev(p1[:7]), ramp=False, first_track=0)
            twin.set_params(p1[:7], ramp=False, first_track=0)
        y = host(plan.process(dev(xs[i].ravel()))).reshape(T, B)
        assert same(y, twin.process(xs[i])) and same_state(plan, twin), i
    cur, tgt = plan.params()
    assert same(host(cur), twin.current) and same(host(tgt), twin.target)
    plan.close()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def refused(gab, call, text):
    with pytest.raises(gab.GabError) as e:
        call()
    assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
    assert str(e.value) == "gab error -1: " + text, str(e.value)


def test_each_refusal_with_its_whole_text(gab):
    import torch
    case = (5, 8, 2, "mid", "cubic")
    T, B, R, pair, curve = case
    Ku, Kd = taps_of(pair, R)
    p0, xs = rows_mix(T, 14), signal(3, T, B, 15)
    for args, text in (((T, B, 3), "oversample must be 1, 2, 4 or 8"),
                       ((T, B, 1, "cubic", 4, 4), "up_taps and down_taps must be 0 at oversample 1"),
                       ((T, B, 2, "cubic", 66, 8), "up_taps must be even and 4..64"),
                       ((T, B, 4, "cubic", 8, 12), "down_taps must be 4..256 and a multiple of 2 * oversample"),
                       ((T, (1 << 20) + 1, 2), "bufsize must be <= 2^20"),
                       ((0, B, 2), "tracks and bufsize must be > 0")):
        refused(gab, lambda: gab.SaturatorPlan(*args), "gab_sat_create: " + text)
    with pytest.raises(ValueError):
        gab.SaturatorPlan(T, B, 2, "tanh")
    plan, twin = make(gab, case, p0), twin_of(case, p0)
    assert same(host(plan.process(dev(xs[0].ravel()))).reshape(T, B), twin.process(xs[0]))
    before = [host(a) for a in plan.state()] + [host(a) for a in plan.params()] + [host(a) for a in plan.taps()]

    for field in range(3):                                       # a row that is not finite: every field, the first named
        for value in (np.nan, np.inf, -np.inf):
            bad = rows_mix(T, 16)
            bad[2, field] = value
            bad[3, 0] = np.nan
            for ramp in (True, False):
                refused(gab, lambda: plan.set_params(dev(bad), ramp=ramp),
                        "gab_sat_set_params: " + st.refused_row(bad))
    bad = rows_mix(2, 16)
    bad[1, 1] = np.inf
    refused(gab, lambda: plan.set_params(dev(bad), first_track=3),
            "gab_sat_set_params_tracks: track 4 field 1 (bias) must be finite; the plan keeps its parameters")
    for first, n in ((-1, 2), (0, 0), (T, 1), (T - 1, 2)):
        rc = gab.lib.gab_sat_set_params_tracks(plan._h, ctypes.c_void_p(dev(bad).data_ptr()), first, n, 1, None)
        assert rc == -1 and gab.lib.gab_last_error().decode() == \
            "gab_sat_set_params_tracks: the track range is outside the plan"

    up, down = twin.up.taps.copy(), twin.down.taps.copy()        # taps that are not finite: both tables are kept
    for table, where in (("up", (1, 3)), ("down", (0, 7)), ("both", None)):
        u, d = up.copy(), down.copy()
        if table in ("up", "both"):
            u[where or (0, 2)] = np.nan
        if table in ("down", "both"):
            d[where or (0, 1)] = np.inf
        refused(gab, lambda: plan.set_taps(dev(u), dev(d.ravel())), "gab_sat_set_taps: " + st.refused_taps(u, d, Ku, Kd))
    one = gab.SaturatorPlan(T, B, 1, "hard")
    some = dev(up)
    ptr = ctypes.c_void_p(some.data_ptr())
    refused(gab, lambda: gab.check(gab.lib.gab_sat_set_taps(one._h, ptr, ptr, None)),
            "gab_sat_set_taps: a plan at oversample 1 has no taps")
    one.close()

    lib, hp = gab.lib, plan._h                                    # overlaps, null pointers, n_buffers
    big = torch.zeros(4 * T * B * R + 8, device="cuda")
    at = lambda off: ctypes.c_void_p(big.data_ptr() + 4 * off)   # noqa: E731
    text = lambda: lib.gab_last_error().decode()                 # noqa: E731
    for off in (0, 1, T * B - 1):
        assert lib.gab_sat_process(hp, at(0), at(off), None) == -1
        assert text() == "gab_sat_process: d_out may not overlap d_in: the output is delayed"
    assert lib.gab_sat_process_batch(hp, at(T * B), at(0), 2, None) == -1
    assert text() == "gab_sat_process_batch: d_out may not overlap d_in: the output is delayed"
    assert lib.gab_sat_apply(hp, at(0), at(1), 1, None) == -1
    assert text() == "gab_sat_apply: d_out may be d_in itself; any other overlap is refused"
    assert lib.gab_sat_apply(hp, at(0), at(R * T * B), 2, None) == -1
    for call, args in (("process", (at(0), None, None)), ("process", (None, at(0), None)),
                       ("process_batch", (None, at(0), 1, None)), ("apply", (at(0), None, 1, None)),
                       ("set_params", (None, 1, None)), ("set_taps", (at(0), None, None)), ("set_taps", (None, at(0), None)),
                       ("info", (None,) * 5), ("params", (None,) * 3), ("state", (None,) * 4)):
        assert getattr(lib, "gab_sat_" + call)(hp, *args) == -1 and text() == "gab_sat_%s: null pointer" % call, call
    for call in ("process_batch", "apply"):
        for n in (0, -2):
            assert getattr(lib, "gab_sat_" + call)(hp, at(0), at(2 * R * T * B), n, None) == -1
            assert text() == "gab_sat_%s: n_buffers must be > 0" % call

    after = [host(a) for a in plan.state()] + [host(a) for a in plan.params()] + [host(a) for a in plan.taps()]
    assert all(same(a, b) for a, b in zip(before, after))         # nothing above touched the plan
    for i in (1, 2):
        assert same(host(plan.process(dev(xs[i].ravel()))).reshape(T, B), twin.process(xs[i])), i
    plan.close()


@pytest.mark.parametrize("name", ["sat"])
def test_entries(gab, monkeypatch, name):
    """The row of tests/test_plan_entries_gpu.py's table for the saturator, through that file's test."""
    import test_plan_entries_gpu as entries
    T, B, bad = entries.T, entries.B, entries.INVALID
    monkeypatch.setitem(entries.PLANS, "sat", (
        (2, 1, 4, 4), [((T, B, 3, 1, 4, 4), bad, "oversample must be 1, 2, 4 or 8"),
                       ((T, B, 2, 3, 4, 4), bad, "curve must be 0 (hard), 1 (cubic) or 2 (rational)"),
                       ((T, B, 1, 1, 4, 4), bad, "up_taps and down_taps must be 0 at oversample 1"),
                       ((T, B, 2, 1, 5, 4), bad, "up_taps must be even and 4..64"),
                       ((T, B, 2, 1, 4, 6), bad, "down_taps must be 4..256 and a multiple of 2 * oversample"),
                       ((T, (1 << 20) + 1, 2, 1, 4, 4), bad, "bufsize must be <= 2^20")],
        "out n", T * B, "gab_sat_params", "null pointer"))
    entries.test_entries(gab, name)


# ---- 4. values at the edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CENSUS[2], WIDE])
def test_a_nan_and_an_infinity_stay_in_their_track_and_leave_it(gab, case):
    T, B, R, pair, curve = case
    Ku, Kd = taps_of(pair, R)
    span = Ku - 1 + -(-(Kd - 1) // R)
    n = 2 + -(-(span + 8) // B)
    p0, xs = rows_mix(T, 17), signal(n, T, B, 18)
    dirty = xs.copy()
    t, last = 40, B + 3
    dirty[0, t, B // 2] = np.nan
    dirty[1, t, 3] = np.inf                                       # stream position B + 3 is the last that is not finite
    clean, plan = make(gab, case, p0), make(gab, case, p0)
    a = host(clean.process_batch(dev(xs.ravel()))).reshape(n, T, B).transpose(1, 0, 2).reshape(T, n * B)
    b = host(plan.process_batch(dev(dirty.ravel()))).reshape(n, T, B).transpose(1, 0, 2).reshape(T, n * B)
    others = np.arange(T) != t
    assert same(a[others], b[others])
    assert not np.isfinite(b[t, B // 2:last + span + 1]).all()                       # it did reach the output
    assert n * B - (last + span + 1) >= 8
    assert same(a[t, last + span + 1:], b[t, last + span + 1:])                      # and is gone behind both windows
    assert all(same(host(u), host(v)) for u, v in zip(clean.state(), plan.state()))
    clean.close()
    plan.close()


def test_a_tail_decaying_through_the_subnormals(gab):
    case = (3, 64, 2, "mid", "cubic")
    T, B = case[:2]
    rows = np.array([[1.0, 0.0, 1.0], [0.5, 0.0, 0.75], [1.5, 2.0 ** -130, 0.5]], F32)
    s = np.arange(4 * B, dtype=np.float64)
    x = (np.array([1.0, -1.0, 1.0])[:, None] * 2.0 ** (-118.0 - s / 6.0)[None, :]).astype(F32)   # down to 2^-160: zeros
    assert (np.abs(x[:, B]) < 2.0 ** -126).all() and x[0, B] != 0 and not x[:, -B // 2:].any()
    xs = x.reshape(T, 4, B).transpose(1, 0, 2)
    plan, twin = make(gab, case, rows), twin_of(case, rows)
    seen = False
    for i in range(4):
        want = twin.process(xs[i])
        seen = seen or bool(((want != 0) & (np.abs(want) < 2.0 ** -126)).any())
        assert same(host(plan.process(dev(xs[i].ravel()))).reshape(T, B), want) and same_state(plan, twin), i
    assert seen                                                   # subnormal outputs were among them
    plan.close()


# ---- 5. a captured graph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SMALL, WIDE, CENSUS[5]])
def test_graph_replay_gives_the_bits_of_plain_calls(gab, case):
    import torch
    p0, p1, xs, ys, hists = reference(case, ramp_at=1)
    T, B = case[:2]
    plan = make(gab, case, p0)
    assert same(host(plan.process(dev(xs[0].ravel()))).reshape(T, B), ys[0])
    plan.set_params(dev(p1))
    assert same(host(plan.process(dev(xs[1].ravel()))).reshape(T, B), ys[1])          # the ramp buffer, by a plain call
    x, out = torch.zeros(T * B, device="cuda"), torch.zeros(T * B, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(x, out)
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same_hist(plan, hists[1])                              # the capture recorded a launch without running it
    for i in range(2, N_CALLS):
        x.copy_(dev(xs[i].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same(host(out).reshape(T, B), ys[i]), i
    assert same_hist(plan, hists[-1])
    del graph
    plan.close()
