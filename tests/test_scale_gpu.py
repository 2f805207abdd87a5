"""The thirteen track plans at their bench shapes, past 2^30, 2^31 and 2^32 elements in one call, and at the largest
calls they accept.  No host twin runs at these sizes; the reference is the contract itself (tests/scale_helpers.py):

  (1) plan A's one process_batch over [n][...] is, bit for bit, plan B's n process calls on a scratch block each.  B's
      pointers are advanced on the host in 64 bits and its kernels see one buffer, so an offset that wraps in A's kernel
      makes A differ from B on the buffers across and above the boundary (tests/test_scale_host.py shows that the block
      a wrapped offset lands in is another block of the fill).  Only A's tensors exist at full size: B's input is made
      again, buffer by buffer, from the fill's seed, and compared at once.
  (2) plan C holds three pieces of plan B's tracks (the first 64, 64 in the middle, the last piece: 3 tracks of 65 539)
      with their rows of every table and their slices of every buffer, and gives B's bits on them.  C is the size of
      plan that the small suites tie to the host twins.

Comparisons are of integer views on the device: no tolerance, two NaNs of the same bits are the same.  Carried state is
compared behind the last buffer, A against B and C against B's rows.  A plan with a ramped table runs each bench case
once more with a ramped set in front.  Every output of A is poisoned (all ones) before the call.

Tiers.  bench: scale_helpers.bench_cases(), 8 192 x 512 x 32, the settings of tools/*_bench.py.  boundary:
scale_helpers.edge_cases() (the table of tensors, n and bytes is in its docstring), in place where the header allows
d_out == d_in.  limits: the largest spectrum call (2^23 workgroups, an input of exactly 2^31 elements) and the refusals
in front of it.  A case's id ends in the device bytes it needs; a case skips only if torch.cuda.mem_get_info shows
fewer free.  Out of scope: one buffer of 2^31 elements or more (no bench or user shape is near it), and the convolution
plans (test_gpu_parity.py holds the batch kernel past 2^30 elements).

What carries the offsets that these cases pass through (read in the kernels; every one is 64 bits):
    eq         ((size_t)n T + track) B + lane M (scan); d_in + n (size_t)(T B) on the host (ordered, a launch a buffer)
    mix        in + (size_t)n T B, dst + ((size_t)n n_groups + grp) M B; the host's d_in + done (size_t)(T B) between
               the launches of a batch; the final pass indexes size_t e = blockIdx.x 64 + lane
    delay      ((size_t)nb T + t) B                      meter      ((size_t)nb T + t0) B, rows ((size_t)nb T + track) 8
    resample   ((size_t)nb T + t0) B and ... OC           dyn, gate, lim, reverb, xover   x + nb (size_t)(T B) (+ K, O)
    spectrum, resynthesis, denoise   ((size_t)nb T + t) B + s with nb, s from an int sample index below 2^31 - 1024
               (the host's check_length); rows ((size_t)f T + t) 513
"""
import ctypes

import numpy as np
import pytest

import scale_helpers as sh
from plan_helpers import gab  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SEED = 29
BENCH, EDGE = sh.bench_cases(), sh.edge_cases()


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def poison(t):
    """All ones in every word: a NaN in a float32, -1 in an int32; nothing a plan writes."""
    import torch
    t.view(torch.int32).fill_(-1)
    return t


class Actor:
    """One plan of a case at T tracks: how it is made, set and run, and where the tracks lie in its blocks."""
    lead_in = lead_out = 1      # dimensions in front of the track dimension of a one-buffer block: [lead][T][...]
    side = None                 # the dtype of a side output [T] per buffer (gr, act)
    offset = 0                  # floats that plan A's tensors lie off 16-byte alignment

    def __init__(self, g, c, T):
        self.g, self.c, self.o, self.T, self.B = g, c, dict(c.opts), T, c.B
        self.plan = self.make()

    def close(self):
        self.plan.close()

    def units(self):
        t = sh.tensors(self.c._replace(T=self.T))
        names = list(t)
        return t[names[0]], t["io"] if "io" in t else t[names[1]]

    def tables(self, seed):
        """name -> numpy [T][...], a row per track."""
        return {}

    def set(self, tabs, ramp):
        pass

    def fill(self, block, seed, i, lv):
        """Block i of the input (or of the key) into a one-buffer block; lv: a level per track [T]."""
        return sh.fill(block.view(self.lead_in, self.T, -1), seed, i, lv[None, :, None])

    def take(self, block, lead, sel):
        return block.view(lead, self.T, -1)[:, sel].contiguous().view(-1)

    def state(self):
        s = self.plan.state()
        return list(s) if isinstance(s, tuple) else [s]


def rows_of(tabs, sel):
    return tabs if sel is None else {k: v[sel] for k, v in tabs.items()}


class Eq(Actor):
    def make(self):
        return self.g.EqPlan(self.T, self.B, self.o["sections"])

    def tables(self, seed):
        """Poles at radius 0.5 .. 0.9 and any angle; zeros that keep a section's gain small."""
        rng = np.random.RandomState(seed)
        S = self.o["sections"]
        r, th = rng.uniform(0.5, 0.9, (self.T, S)), rng.uniform(0.0, np.pi, (self.T, S))
        a1, a2 = -2.0 * r * np.cos(th), r * r
        return {"coeffs": np.stack([0.5 + 0.0 * r, 0.25 * a1, 0.125 * a2, a1, a2], axis=-1).astype(np.float32)}

    def set(self, tabs, ramp):
        self.plan.set_coeffs(dev(tabs["coeffs"]))

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, out=out)

    def one(self, x, out, key, side):
        self.plan.process(x, out=out)


class EqSeq(Eq):
    """The ordered form: plan A's batch lies 4 bytes off 16-byte alignment, which takes the sequential kernel, a launch
    a buffer from host pointers; plan B and C call process_sequential."""
    offset = 1

    def batch(self, x, n, out, key, side):
        assert x.data_ptr() % 16 == 4
        self.plan.process_batch(x, out=out)

    def one(self, x, out, key, side):
        self.plan.process(x, out=out, sequential=True)


class Mix(Actor):
    def make(self):
        return self.g.MixPlan(self.T, self.B, self.o["buses"])

    def tables(self, seed):
        g = np.random.RandomState(seed).uniform(0.25, 1.0, (self.T, self.o["buses"]))        # finite, no zero
        return {"gains": (g * np.where(np.arange(self.T)[:, None] % 3 == 0, -1.0, 1.0)).astype(np.float32)}

    def set(self, tabs, ramp):
        self.plan.set_gains(dev(tabs["gains"]), ramp=ramp)

    def fill(self, block, seed, i, lv):
        if self.o["layout"] == "sample":
            return sh.fill(block.view(self.B, self.T), seed, i, lv[None, :])
        return super().fill(block, seed, i, lv)

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, out=out, layout=self.o["layout"])

    def one(self, x, out, key, side):
        self.plan.process(x, out=out, layout=self.o["layout"])

    def state(self):
        return list(self.plan.gains())


class Delay(Actor):
    def make(self):
        return self.g.DelayPlan(self.T, self.B, self.o["max_delay"], self.o["interp"])

    def tables(self, seed):
        rng, T = np.random.RandomState(seed), self.T
        d = rng.uniform(self.plan.min_delay, self.o["max_delay"], T)
        return {"params": np.stack([d, rng.uniform(-0.75, 0.75, T), rng.uniform(-1, 1, T), rng.uniform(-1, 1, T)],
                                   axis=-1).astype(np.float32)}

    def set(self, tabs, ramp):
        self.plan.set_params(dev(tabs["params"]), ramp=ramp)

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, out=out)

    def one(self, x, out, key, side):
        self.plan.process(x, out=out)

    def state(self):
        return list(self.plan.line()) + list(self.plan.params())


class Meter(Delay):
    def make(self):
        p = self.g.MeterPlan(self.T, self.B, self.o["window"])
        p.set_decay(0.75)
        return p

    def tables(self, seed):
        return {}

    def set(self, tabs, ramp):
        pass

    def state(self):
        return Actor.state(self)


class Resample(Meter):
    def make(self):
        return self.g.ResamplePlan(self.T, self.B, self.o["up"], self.o["down"], self.o["taps"])

    def batch(self, x, n, out, key, side):
        self.counts = self.plan.process_batch(x, out=out)[1]

    def one(self, x, out, key, side):
        self.counts = getattr(self, "counts", []) + [self.plan.process(x, out=out)[1]]


class Dyn(Actor):
    def make(self):
        import torch
        self.side = torch.float32
        return self.g.DynamicsPlan(self.T, self.B, link=self.o["link"])

    def tables(self, seed):
        rng, T = np.random.RandomState(seed), self.T
        return {"params": self.g.dynamics_params(rng.uniform(-30, -6, T), rng.uniform(1.5, 8.0, T), 6.0,
                                                 rng.uniform(1, 20, T), rng.uniform(50, 200, T), rng.uniform(0, 6, T))}

    def set(self, tabs, ramp):
        self.plan.set_params(dev(tabs["params"]), ramp=ramp)

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, key=key, out=out, gr=side)

    def one(self, x, out, key, side):
        self.plan.process(x, key=key, out=out, gr=side)


class Gate(Dyn):
    def make(self):
        import torch
        self.side = torch.int32
        return self.g.GatePlan(self.T, self.B, link=self.o["link"])

    def tables(self, seed):
        rng, T = np.random.RandomState(seed), self.T
        return {"params": self.g.gate_params(rng.uniform(-30, -10, T), None, rng.uniform(0.5, 5, T), rng.uniform(20, 200, T),
                                             rng.uniform(0, 20, T), range_db=rng.uniform(-60, -20, T))}

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, key=key, out=out, act=side)

    def one(self, x, out, key, side):
        self.plan.process(x, key=key, out=out, act=side)


class Lim(Dyn):
    def make(self):
        import torch
        self.side = torch.float32
        return self.g.LimiterPlan(self.T, self.B, self.o["lookahead"], self.o["link"])

    def tables(self, seed):
        rng, T = np.random.RandomState(seed), self.T
        return {"params": self.g.limiter_params(rng.uniform(-18, -3, T), rng.uniform(20, 200, T), rng.uniform(0, 6, T))}

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, out=out, gr=side)

    def one(self, x, out, key, side):
        self.plan.process(x, out=out, gr=side)


class Reverb(Delay):
    def make(self):
        o = self.o
        return self.g.ReverbPlan(self.T, self.B, lines=o["lines"], outs=o["outs"], max_delay=o["max_delay"])

    def tables(self, seed):
        rng, T, o = np.random.RandomState(seed), self.T, self.o
        d = rng.randint(32, o["max_delay"] + 1, (T, o["lines"]))
        rt60 = rng.uniform(0.3, 2.0, T)
        delays, table = self.g.reverb_params(rt60, 0.5 * rt60, lines=o["lines"], outs=o["outs"],
                                             wet_db=rng.uniform(-12, 0, T), dry_db=rng.uniform(-6, 0, T), delays=d)
        return {"delays": delays, "params": table}

    def set(self, tabs, ramp):
        if not ramp:
            self.plan.set_delays(dev(tabs["delays"]))
        self.plan.set_params(dev(tabs["params"]), ramp=ramp)

    def state(self):
        return Actor.state(self) + list(self.plan.params())


class Xover(Delay):
    def make(self):
        self.lead_out = self.o["bands"]
        return self.g.CrossoverPlan(self.T, self.B, self.o["bands"])

    def tables(self, seed):
        K = self.o["bands"]
        edges = np.geomspace(20.0, 20000.0, K)
        u = np.random.RandomState(seed).uniform(0.02, 0.98, (self.T, K - 1))
        return {"rows": self.g.crossover_rows(edges[:-1] * (edges[1:] / edges[:-1]) ** u)}

    def set(self, tabs, ramp):
        self.plan.set_splits(dev(tabs["rows"]))

    def state(self):
        return Actor.state(self)


class Spec(Meter):
    def make(self):
        o = self.o
        self.lead_out = self.fpb = self.B // o["hop"]
        p = self.g.SpectrumPlan(self.T, self.B, o["hop"], o["mode"], o["bands"])
        if o["bands"] > 1:
            p.set_bands(self.g.spectrum_band_edges(o["bands"]))
        return p

    def batch(self, x, n, out, key, side):
        assert self.plan.process_batch(x, out=out).shape[0] == n * self.fpb

    def one(self, x, out, key, side):
        assert self.plan.process(x, out=out).shape[0] == self.fpb


class Resyn(Meter):
    def make(self):
        self.lead_in = self.B // self.o["hop"]
        return self.g.ResynthesisPlan(self.T, self.B, self.o["hop"])

    def batch(self, x, n, out, key, side):
        self.plan.process_batch(x, n, out=out)

    def one(self, x, out, key, side):
        self.plan.process(x, out=out)


class Dn(Delay):
    def make(self):
        return self.g.DenoisePlan(self.T, self.B, self.o["hop"])

    def tables(self, seed):
        rng, T = np.random.RandomState(seed), self.T
        return {"thr": (10.0 ** rng.uniform(-8, -3, (T, sh.BINS))).astype(np.float32),
                "params": self.g.denoise_params(rng.uniform(-30, -6, T), rng.uniform(1, 10, T), rng.uniform(20, 100, T),
                                                hop=self.o["hop"])}

    def set(self, tabs, ramp):
        self.plan.set_thresholds(dev(tabs["thr"]))
        self.plan.set_params(dev(tabs["params"]))

    def state(self):
        return Actor.state(self)


class DnRows(Dn):
    """The gate alone: plan A takes every frame in one call, plan B and C a frame a call."""

    def batch(self, x, n, out, key, side):
        self.plan.process_rows(x, out=out)

    def one(self, x, out, key, side):
        self.plan.process_rows(x, out=out)


ACTORS = {"eq": Eq, "eqseq": EqSeq, "mix": Mix, "delay": Delay, "meter": Meter, "resample": Resample, "dyn": Dyn,
          "gate": Gate, "lim": Lim, "reverb": Reverb, "xover": Xover, "spec": Spec, "resyn": Resyn, "dn": Dn,
          "dnrows": DnRows}


def same_state(a, b, sel=None, T=None):
    """The carried state of two plans, item by item; sel: b's rows of those tracks (an item with a row per track)."""
    import torch
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        if not isinstance(u, torch.Tensor):
            assert u == v, i
            continue
        if sel is not None and v.shape[0] == T:
            v = v[sel]
        assert u.shape == v.shape and sh.same_bits(u, v), "state item %d differs" % i


def hold(g, c, ramp=False, spoil=None):
    """Oracle (1) and oracle (2) on case c; ramp: a ramped set of every table in front of the first buffer.  spoil: a
    buffer of plan A's output in which one bit is flipped behind the call (the harness's own control)."""
    import torch
    torch.cuda.empty_cache()
    free, need = torch.cuda.mem_get_info()[0], sh.need_bytes(c)
    if free < need:
        pytest.skip("needs %d bytes of device memory, %d are free" % (need, free))
    torch.cuda.reset_peak_memory_stats()
    cls, T, n = ACTORS[c.plan], c.T, c.n
    sel_np = sh.shard_tracks(T) if sh.owner_tracks(c) is not None else None
    sel = None if sel_np is None else torch.from_numpy(sel_np).cuda()
    actors = []
    try:
        A, Bp = cls(g, c, T), cls(g, c, T)
        actors += [A, Bp]
        C = None
        if sel is not None:
            C = cls(g, c, len(sel_np))
            actors.append(C)
        for k in range(2 if ramp else 1):
            tabs = A.tables(SEED + k)
            for P in actors:
                P.set(rows_of(tabs, sel_np if P is C else None), ramp=k == 1)
        del tabs
        lv = sh.levels(T, "cuda")
        uin, uout = A.units()
        names = sh.tensors(c)
        in_place, keyed = "io" in names, "key" in names
        store = torch.empty(n * uin + 4, device="cuda")
        x = store[A.offset:A.offset + n * uin]
        for i in range(n):
            A.fill(x[i * uin:(i + 1) * uin], SEED, i, lv)
        key = None
        if keyed:
            key = torch.empty(n * uin, device="cuda")
            for i in range(n):
                A.fill(key[i * uin:(i + 1) * uin], SEED + 1, i, lv)
        out = x if in_place else poison(torch.empty(n * uout, device="cuda"))
        side = None if A.side is None else poison(torch.empty(n * T, dtype=A.side, device="cuda"))
        A.batch(x, n, out, key, side)
        if spoil is not None:
            out.view(torch.int32)[(spoil + 1) * uout - 1] ^= 1
        if c.plan == "mix" and c.T == sh.EDGE_T:
            launches_and_groups(A, c)

        sx, so = torch.empty(uin, device="cuda"), torch.empty(uout, device="cuda")
        kx = torch.empty(uin, device="cuda") if keyed else None
        ss = None if A.side is None else torch.empty(T, dtype=A.side, device="cuda")
        if C is not None:
            co = torch.empty(C.units()[1], device="cuda")
            cs = None if A.side is None else torch.empty(C.T, dtype=A.side, device="cuda")
        bad = torch.zeros(n, 4, dtype=torch.bool, device="cuda")
        for i in range(n):
            A.fill(sx, SEED, i, lv)
            if keyed:
                A.fill(kx, SEED + 1, i, lv)
            poison(so)
            Bp.one(sx, so, kx, ss)
            bad[i, 0] = sh.differs(so, out[i * uout:(i + 1) * uout])
            if ss is not None:
                bad[i, 1] = sh.differs(ss, side[i * T:(i + 1) * T])
            if C is not None:
                poison(co)
                C.one(A.take(sx, A.lead_in, sel), co, None if kx is None else A.take(kx, A.lead_in, sel), cs)
                bad[i, 2] = sh.differs(co, A.take(so, A.lead_out, sel))
                if cs is not None:
                    bad[i, 3] = sh.differs(cs, ss[sel])
        bad = bad.cpu().numpy()
        for col, what in enumerate(("the batch's output differs from the per-buffer calls'",
                                    "the batch's side output differs from the per-buffer calls'",
                                    "the shard's output differs from the whole plan's",
                                    "the shard's side output differs from the whole plan's")):
            assert not bad[:, col].any(), "%s on buffers %s" % (what, np.flatnonzero(bad[:, col]).tolist())
        if c.plan == "resample":
            want = g.ResamplePlan.counts(c.B, A.o["up"], A.o["down"], 0, n)
            assert A.counts == want and Bp.counts == want and C.counts == want
        same_state(A.state(), Bp.state())
        if C is not None:
            same_state(C.state(), Bp.state(), sel, T)
        print("\nscale %s%s: peak of torch allocations %.2f GiB" % (
            sh.case_id(c), " ramped" if ramp else "", torch.cuda.max_memory_allocated() / 2.0 ** 30))
    finally:
        for P in actors:
            P.close()
        store = x = key = out = side = sx = so = kx = ss = co = cs = None
        torch.cuda.empty_cache()


def launches_and_groups(A, c):
    """The mix plan's boundary case took more than one launch and a second pass through the final kernel's rows: from
    plan.form and the shapes, as gab_mix_create works it out (a workspace of 32 MiB of partial sums, 64 buffers a launch
    at the most; kMixRows = 128 rows a pass)."""
    leaf, leaves = A.plan.form
    groups = -(-c.T // (leaf * leaves))
    per_buffer = groups * A.o["buses"] * c.B * 4
    part_buffers = min(max((32 << 20) // per_buffer, 1), 64)
    assert leaf * leaves == 256 and groups > 128
    assert -(-c.n // part_buffers) > 1
    firsts = list(range(0, c.n, part_buffers))                       # the launches start at these buffers
    u = c.T * c.B
    for b in sh.BOUNDARIES:                                          # and a launch itself lies across or above each boundary
        assert any(f * u >= b or f * u < b < min(f + part_buffers, c.n) * u for f in firsts)


# ---- the bench tier ----
@pytest.mark.parametrize("c", BENCH, ids=[sh.case_id(c) for c in BENCH])
def test_bench_shape(gab, c):
    hold(gab, c)


def test_the_harness_sees_one_flipped_bit(gab):
    c = [c for c in BENCH if c.plan == "delay"][0]
    with pytest.raises(AssertionError, match=r"the batch's output differs from the per-buffer calls' on buffers \[17\]"):
        hold(gab, c, spoil=17)


RAMPED = [c for c in BENCH if c.plan in sh.RAMPED]


@pytest.mark.parametrize("c", RAMPED, ids=[sh.case_id(c) for c in RAMPED])
def test_bench_shape_behind_a_ramped_set(gab, c):
    hold(gab, c, ramp=True)


# ---- the boundary tier ----
@pytest.mark.parametrize("c", EDGE, ids=[sh.case_id(c) for c in EDGE])
def test_past_two_to_the_32_elements(gab, c):
    """scale_helpers.edge_cases() has the table: plan, tensor, n, bytes."""
    hold(gab, c)


# ---- the limits tier ----
def refused(gab, rc, text):
    assert rc == gab._capi.GAB_ERR_INVALID_ARG and gab.lib.gab_last_error().decode() == text, (rc, gab.lib.gab_last_error())


def test_the_largest_spectrum_call_and_the_first_refused(gab):
    """T = 65 536, hop 32, B = 1 024, n = 32, one band: frames x groups = 1 024 x 8 192 = 2^23 workgroups exactly, 2^31
    threads in one launch, the input exactly 2^31 elements (8 GiB; the band rows 256 MiB).  Accepted, and the rows are
    the per-buffer calls' and the shard's.  33 buffers are 1 056 frames: refused in front of the launch (spectrum_launch
    compares before it reads a pointer, so the call is made with two small tensors), and the plan has not moved."""
    import torch
    c = sh.SPEC_LIMIT
    hold(gab, c)
    plan = gab.SpectrumPlan(c.T, c.B, 32, "power", 1)
    try:
        x = sh.fill(torch.empty(c.T * c.B, device="cuda"), SEED, 0)
        plan.process(x)                                              # a history that is not zero
        before = plan.state()
        small, f = torch.zeros(64, device="cuda"), ctypes.c_int(-7)
        refused(gab, gab.lib.gab_spec_process_batch(plan._h, ctypes.c_void_p(small.data_ptr()), ctypes.c_void_p(small.data_ptr()),
                                                    33, ctypes.byref(f), None),
                "gab_spec_process_batch: more than 2^23 workgroups (frames x tracks / 8) in one call")
        after = plan.state()
        assert f.value == -7 and after[2] == before[2] and sh.same_bits(after[0], before[0]) and sh.same_bits(after[1], before[1])
        assert not small.any()
    finally:
        plan.close()


def test_one_frame_more_than_the_spectrum_plan_launches_is_refused(gab):
    """A buffer of 1 025 hops at 65 536 tracks: 1 025 frames x 8 192 groups, one frame more than 2^23 workgroups; a
    buffer of 1 024 hops is not refused by the count (its frames() says 1 024, and the call above ran that many)."""
    import torch
    small, f = torch.zeros(64, device="cuda"), ctypes.c_int(-7)
    p = ctypes.c_void_p(small.data_ptr())
    plan = gab.SpectrumPlan(65536, 1025 * 32, 32, "power", 1)
    try:
        assert plan.frames(1) == 1025
        before = plan.state()
        refused(gab, gab.lib.gab_spec_process(plan._h, p, p, ctypes.byref(f), None),
                "gab_spec_process: more than 2^23 workgroups (frames x tracks / 8) in one call")
        after = plan.state()
        assert f.value == -7 and after[2] == before[2] == 0 and sh.same_bits(after[0], before[0]) and not small.any()
    finally:
        plan.close()


def test_the_refusals_of_length(gab):
    """check_length (n B at 2^31 - 1 024: a frame's samples are indexed in an int, up to 1 024 past the call's last) and
    capacity (ceil(n B / hop) above an int) of the spectrum plan; both come before any launch and any access, so the
    tensors are small.  The resynthesis and the denoise plan's check_length are in their own suites; capacity of the
    resynthesis plan is here."""
    import torch
    small, f = torch.zeros(64, device="cuda"), ctypes.c_int(-7)
    p = ctypes.c_void_p(small.data_ptr())
    spec, resyn = gab.SpectrumPlan(2, 1024, 512), gab.ResynthesisPlan(2, 1024, 512)
    try:
        before = spec.state()
        n = ((1 << 31) - 1024) // 1024                               # n B = 2^31 - 1024: the first length refused
        refused(gab, gab.lib.gab_spec_process_batch(spec._h, p, p, n, ctypes.byref(f), None),
                "gab_spec_process_batch: n_buffers * bufsize must be below 2^31 - 1024")
        assert f.value == -7 and spec.state()[2] == before[2] and sh.same_bits(spec.state()[0], before[0])
        assert spec.frames(n - 1) == (n - 1) * 2                     # one buffer fewer is a length the plan counts
        for plan, who in ((spec, "gab_spec_frames"), (resyn, "gab_resyn_frames")):
            plan.close()
        spec, resyn = gab.SpectrumPlan(1, 1 << 20, 32), gab.ResynthesisPlan(1, 1 << 20, 32)
        cap = ctypes.c_int(-7)
        for fn, plan, who in ((gab.lib.gab_spec_frames, spec, "gab_spec_frames"),
                              (gab.lib.gab_resyn_frames, resyn, "gab_resyn_frames")):
            refused(gab, fn(plan._h, 1 << 16, ctypes.byref(cap)), who + ": n_buffers * bufsize is too large")
            assert cap.value == -7
            assert fn(plan._h, (1 << 16) - 1, ctypes.byref(cap)) == 0 and cap.value == ((1 << 16) - 1) << 15
            cap.value = -7
        assert not small.any()
    finally:
        spec.close()
        resyn.close()


def test_the_mix_plan_refuses_a_launch_it_cannot_index(gab):
    """gab_mix_create: groups x ceil(bufsize / 64) above an int is refused before anything is allocated.  The
    largest shape below it in tracks is accepted by the same rule (not created here: its gains alone are 8 GiB).
    gab_mix_process_batch's "the batch is too large for one launch" cannot be reached: a launch takes at most
    part_buffers buffers, whose partial sums fit 32 MiB, or one buffer of buses x bufsize <= 64 x (2^31 - 1) sums, and
    either is below 2^31 x 64 outputs.  (It also stands behind the first kernel's launch, so it is no refusal "before
    any launch" and nothing here calls for it.)"""
    h = ctypes.c_void_p()
    T = (1 << 31) - 1                                                # 2^23 groups of 256 tracks
    refused(gab, gab.lib.gab_mix_create(ctypes.byref(h), T, 64 * 256 + 1, 1),
            "gab_mix_create: tracks x bufsize is too large for one launch")
    assert not h.value
