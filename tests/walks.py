"""Seeded random walks of calls over ten track plans: the nine bit-exact ones (mix, delay, meter, resample, dynamics,
reverb, gate, limiter and crossover) and the spectrum plan, whose framing and carried state are exact.  A plain helper
module like plan_helpers.py: tests/test_walks_host.py shows on the CPU that the walks reach the orderings they are for
and catch a twin with one seeded defect; tests/test_walks_gpu.py replays them on the device.

walk(plan, shape, seed, steps) drives test_edges_host's Tape over the plan's host actor with a RandomState(seed) and
returns what test_edges_host._reference returns: (ops, outputs per buffer, the state at the end, the host actor), cached
and read only.  Beside the calls the actors already had, a tape holds

    params_tracks / gains_tracks / delays_tracks (table, first_track[, ramp])   a set of a range of tracks
    refused(table, first_track, ramp)   a table with a value outside the plan's rule: refused, nothing changes
    taps(table)                         resample: set_taps mid-stream, the designed table and a one-hot one in turn
    splits / splits_tracks (rows[, first_track])   crossover: a set, never ramped; refused(rows, first_track)
    unset_run(x)                        crossover: a run on a plan that has no rows yet: refused, nothing changes
    window(w) / edges(e)                spectrum: set_window and set_bands mid-stream
    refused_window(w) / refused_edges(e)   spectrum: a window with a value that is not finite or a zero sum, edges that
                                        do not ascend inside 0..513: refused, nothing changes
    ("cut",)                            a marker: play(batch=True) ends the current batch here
    ("check", state)                    a marker behind every set, refused set and reset and at the end: the host actor's
                                        carried state there, which a device actor compares its own with

How a walk is drawn.  The orderings a walk is for (a range set on a pending ramp, a refused set and a reset on one, two
ramped sets before a buffer, a ramp at the head of a batch and between two batches, a steady batch of three buffers or
more; resample: a batch across the end of the period, more buffers than a period behind a reset; limiter: a loud
buffer, a cut, quiet buffers, so that a held minimum and a running release cross a call; crossover: the opening on a
plan without rows, a set between two batches and between two buffers, on a state that is not zero; spectrum: a reset
off the hop grid, a window between two batches, a batch that emits no frame and one that emits more frames than it has
buffers) are short scenes of
two to six calls.  The seed draws the order of the scenes, every range, table, key and cut in them, and the calls
between them: one call of the plan's vocabulary at a time, until the walk has `steps` calls (the check markers not
counted) or 24 buffers.  census(ops) reads all of that back from the tape alone, with a model of `pending` that knows
only: a ramped set raises it, a buffer and a reset drop it."""
import collections
import functools

import numpy as np

import spectrum_twin as st
from limiter_twin import levels as lim_levels
from limiter_twin import lim_mix
from test_crossover_host import rows32 as xover_rows32
from test_delay_host import delay_mix
from test_dynamics_host import dyn_mix
from test_edges_host import HOSTS, Tape, lvl
from test_gate_host import bursts, gate_mix
from test_mix_host import gains
from test_resample_host import reduced, resample_taps32
from test_reverb_host import MIN_DELAY as REVERB_MIN_DELAY
from test_reverb_host import reverb_mix

Walk = collections.namedtuple("Walk", "plan shape seed steps")
MAX_BUFFERS = 24
MAX_BATCH = 5
RAMPED = ("mix", "delay", "dyn", "reverb", "gate", "lim")    # the plans with a ramped table (RampedTable in gab_plan.hpp)
KEYED = ("dyn", "gate")
SETS = ("params", "gains", "params_tracks", "gains_tracks")  # the sets that take `ramp` as their last argument

# Shapes as in test_edges_host.CASES; gate: (tracks, bufsize, link, keyed).  Per plan: 130 tracks (reverb: 34 x 4 and
# 9 x 16 lines) end inside an owner of 64, one count is 64 or less; bufsize 100 ends in a short chunk, 128 takes the
# vector forms, 7 is below a chunk.  Resample: 7/3 has M/L = 2 with M mod L = 1 and a period of 3 at bufsize 100; 2/5 a
# period of 5 at bufsize 7; 1/1024 a period of 8 at bufsize 128, seven of them without an output; 64/1 the largest table.
WALKS = [
    Walk("mix", (130, 100, 2, "track"), 101, 40),
    Walk("mix", (130, 128, 33, "sample"), 102, 40),
    Walk("mix", (40, 7, 33, "track"), 103, 40),
    Walk("mix", (64, 128, 2, "sample"), 104, 40),
    Walk("delay", (130, 100, 64, "linear"), 111, 40),
    Walk("delay", (130, 128, 64, "lagrange3"), 112, 40),
    Walk("delay", (50, 7, 20, "lagrange3"), 113, 40),
    Walk("delay", (64, 128, 64, "linear"), 114, 40),
    Walk("meter", (130, 100, 3), 121, 40),
    Walk("meter", (130, 128, 3), 122, 40),
    Walk("meter", (20, 7, 5), 123, 40),
    Walk("meter", (64, 128, 1), 124, 40),
    Walk("resample", (130, 100, 7, 3, 12), 131, 40),
    Walk("resample", (3, 128, 1, 1024, 4), 132, 40),
    Walk("resample", (66, 7, 2, 5, 16), 133, 40),
    Walk("resample", (2, 7, 64, 1, 256), 134, 40),
    Walk("dyn", (130, 100, 1, True), 141, 40),
    Walk("dyn", (130, 128, 2, False), 142, 40),
    Walk("dyn", (60, 7, 2, True), 143, 40),
    Walk("dyn", (64, 128, 1, False), 144, 40),
    Walk("reverb", (34, 100, 4, 2, 64), 151, 40),
    Walk("reverb", (9, 128, 16, 1, 64), 152, 40),
    Walk("reverb", (34, 7, 4, 1, 64), 153, 40),
    Walk("reverb", (17, 128, 8, 2, 64), 154, 40),
    Walk("gate", (130, 100, 1, True), 161, 40),
    Walk("gate", (128, 128, 64, False), 162, 40),
    Walk("gate", (48, 7, 16, True), 163, 40),
    Walk("gate", (68, 100, 4, False), 164, 40),
    # lim: (tracks, bufsize, W, link).  A wave owns 8 tracks.  link 64 and 16 take the detector launch in front, 16 the
    # narrowest that does and in scalar loads; link 8 is the widest group inside the wave, with buffers shorter than
    # W - 1 at k = 7; k = 8 in 16-byte loads.
    Walk("lim", (130, 100, 32, 2), 171, 40),
    Walk("lim", (128, 128, 256, 64), 172, 40),
    Walk("lim", (24, 7, 128, 8), 173, 40),
    Walk("lim", (48, 100, 64, 16), 174, 40),
    # xover: (tracks, bufsize, bands).  A wave owns 64 / G tracks, G = 1, 2, 4 for 2, 3, 4 bands.
    Walk("xover", (130, 100, 2), 181, 40),
    Walk("xover", (70, 128, 3), 185, 40),
    Walk("xover", (40, 7, 4), 183, 40),
    Walk("xover", (33, 128, 4), 184, 40),
    # spec: (tracks, bufsize, hop, mode, bands).  A wave owns a pair of tracks, a workgroup eight tracks.  bufsize 7 at
    # hop 32: most calls emit nothing; 1536 at hop 1000: a call emits one or two frames and is longer than the history.
    Walk("spec", (17, 100, 96, "complex", 0), 191, 40),
    Walk("spec", (9, 128, 256, "power", 31), 192, 40),
    Walk("spec", (3, 7, 32, "power", 0), 193, 40),
    Walk("spec", (2, 1536, 1000, "power", 4), 194, 40),
]


def walk_id(w):
    return "-".join([w.plan] + [str(v) for v in w.shape] + ["seed%d" % w.seed])


def set_name(plan):
    return "gains" if plan == "mix" else "params"


def owner_tracks(plan, shape):
    """Tracks of one owner: a workgroup's 64; for the reverb plan a wave's 64 / lines, for the limiter a wave's 8, for
    the crossover a wave's 64 / G (G = 1, 2, 4 lanes a track for 2, 3, 4 bands), for the spectrum plan a wave's pair."""
    if plan == "reverb":
        return 64 // shape[2]
    if plan == "xover":
        return 64 >> (shape[2] - 2)
    return {"lim": 8, "spec": 2}.get(plan, 64)


def xover_rows(T, K, seed):
    """[T][K - 1][3]: every track its own ascending splits, split j inside the j-th of K - 1 equal parts (in octaves)
    of 20 Hz .. 20 kHz."""
    edges = np.geomspace(20.0, 20000.0, K)
    u = np.random.RandomState(seed).uniform(0.02, 0.98, (T, K - 1))
    return np.stack([xover_rows32(row) for row in edges[:-1] * (edges[1:] / edges[:-1]) ** u])


def window_kind(w):
    w = np.asarray(w, np.float32)
    if np.array_equal(w, st.window_hann()):
        return "hann"
    return "one-hot" if np.count_nonzero(w) == 1 else "positive"


def one_hot_taps(L, K):
    """Row p is 1.0 at j = (3 p) mod K: tests/test_resample_gpu.py's table."""
    t = np.zeros((L, K), np.float32)
    t[np.arange(L), (3 * np.arange(L)) % K] = 1.0
    return t


class Draw:
    """One walk being drawn: the tape, the seed's generator, and what the next draw depends on."""

    def __init__(self, plan, shape, seed, steps):
        self.plan, self.shape, self.steps = plan, shape, steps
        self.T, self.B = shape[0], shape[1]
        self.rng = np.random.RandomState(seed)
        self.host = HOSTS[plan](*shape)
        self.tape = Tape(self.host)
        self.buffers = self.calls = self.batch = 0
        self.pending = []                    # the ranges whose ramp is pending
        self.key = False
        if plan == "resample":
            self.L, self.M = reduced(shape[2], shape[3])
            self.period, self.k, self.hot = self.host.twin.period, 0, False
        self.p = self.windows = 0            # spec: samples since the reset, windows set so far

    # ---- what a call is made of ----
    def table(self):
        plan, s, seed = self.plan, self.shape, int(self.rng.randint(1 << 20))
        if plan == "mix":
            return gains(self.T, s[2], seed)
        if plan == "delay":
            return delay_mix(self.T, self.B, s[2], s[3], seed)
        if plan == "dyn":
            return dyn_mix(self.T, seed)
        if plan == "gate":
            return gate_mix(self.T, seed)
        if plan == "lim":
            return lim_mix(self.T, seed)
        if plan == "xover":
            return xover_rows(self.T, s[2], seed)
        return reverb_mix(self.T, s[2], s[3], seed)

    def block(self, level=None):
        """A buffer: bursts for the keyed plans (level: all of it scaled, so that linked detectors fall silent too);
        for the limiter noise at a level per track between -36 and +12 dB."""
        if self.plan == "lim":
            x = lim_levels(self.T, self.B, int(self.rng.randint(1 << 20)))
            return x if level is None else x * np.float32(level)
        if self.plan in KEYED:
            x = bursts(self.T, self.B, int(self.rng.randint(1 << 20)))
            return x if level is None else x * np.float32(level)
        return lvl(self.rng, (self.T, self.B), 0)

    def range(self, kind):
        """(first, n).  inside: begins and ends inside one owner; span: begins in one owner and ends inside the next;
        overlap: begins inside a range whose ramp is pending, behind its first row, and ends where it likes."""
        T, own, rng = self.T, owner_tracks(self.plan, self.shape), self.rng
        if kind == "overlap" and self.pending:
            a, n = self.pending[int(rng.randint(len(self.pending)))]
            last = min(a + n - 1, T - 2)                               # two tracks at least, the first behind a
            if last > a:
                first = a + 1 + int(rng.randint(last - a))
                return first, 2 + int(rng.randint(T - first - 1))
        if kind == "span" and T > own + 1:
            o = int(rng.randint((T - 2) // own))                       # owner o + 1 holds a track at least
            first = o * own + 1 + int(rng.randint(own - 1))
            end = min((o + 1) * own + 1 + int(rng.randint(max(own - 1, 1))), T)
            return first, end - first
        o = int(rng.randint((T + own - 1) // own))
        lo, hi = o * own, min((o + 1) * own, T)
        if hi - lo < 4:
            return lo, hi - lo                                         # (an owner of three tracks or fewer: all of it)
        first = lo + 1 + int(rng.randint(hi - lo - 3))
        return first, 2 + int(rng.randint(hi - 2 - first))

    def bad_table(self, first, n):
        """Rows [first, first + n) of a good table with one value the rule refuses, and a NaN behind it."""
        plan, s, rng = self.plan, self.shape, self.rng
        p = self.table()[first:first + n].copy()
        W = p.shape[1]
        spots = [(f, v) for f in range(W) for v in (np.nan, np.inf, -np.inf)]
        if plan == "delay":
            spots += [(0, s[2] + 1.0), (0, 0.5), (1, 1.0), (1, -1.0)] * 3
        if plan == "dyn":
            spots += [(1, 0.5), (2, -1.0), (3, -1.0), (4, 1.0), (5, 1.0), (7, 1.0)] * 3
        if plan == "gate":
            spots += [(0, -1.0), (2, 1.0), (3, 1.0), (4, 257.0), (6, 2.5), (6, -1.0)] * 3
        if plan == "reverb":
            spots += [(0, 1.0), (s[2] - 1, -1.0), (s[2], 1.0), (2 * s[2] - 1, -0.5)] * 3
        if plan == "lim":
            spots += [(0, -1.0), (0, 2.0 ** 33), (1, 0.0), (1, 2.0 ** -33), (1, 2.0 ** 33), (2, -0.5), (2, 1.5)] * 3
        f, v = spots[int(rng.randint(len(spots)))]
        r = int(rng.randint(n))
        p[r, f] = v
        later = r * W + f + 1 + int(rng.randint(W))
        if later < p.size:
            p.ravel()[later] = np.nan
        return p

    # ---- the calls ----
    def count(self):
        self.calls += 1
        self.batch = 0
        self.key = self.plan in KEYED and self.shape[3] and bool(self.rng.randint(2))

    def check(self):
        self.tape.check(self.host.state())

    def run(self, level=None):
        if self.buffers >= MAX_BUFFERS:
            return
        if self.plan == "resample" and self.batch:
            # the batch that holds buffer period - 1 goes on into buffer 0 (a period of 1: every batch of two does)
            if self.k == self.period - 1 and self.batch >= MAX_BATCH - 1 and self.period > 1:
                self.cut()
        if self.batch >= MAX_BATCH:
            self.cut()
        if level is None and self.plan in KEYED:
            level = (None, None, 0.25, 0.015625)[int(self.rng.randint(4))]
        x = self.block(level)
        self.tape.run(x, self.block(level) if self.key else None)
        self.buffers, self.calls, self.batch = self.buffers + 1, self.calls + 1, self.batch + 1
        self.pending = []
        self.p += self.B
        if self.plan == "resample":
            self.k = (self.k + 1) % self.period

    def runs(self, n, cuts=True):
        for _ in range(n):
            wrap = self.plan == "resample" and self.k == 0 and self.batch
            if cuts and self.batch and not wrap and self.rng.randint(4) == 0:
                self.cut()
            self.run()

    def cut(self):
        self.tape.cut()
        self.count()

    def set(self, ramp, kind=None):
        """kind None: the whole table; else a range of that kind."""
        name = set_name(self.plan)
        if kind is None:
            getattr(self.tape, name)(self.table(), ramp)
            first, n = 0, self.T
        else:
            first, n = self.range(kind)
            for _ in range(20):                  # (a range of one track, or at the plan's end, cannot be overlapped in part)
                if n >= 2 and (kind == "overlap" or first < self.T - 2):
                    break
                first, n = self.range(kind)
            getattr(self.tape, name + "_tracks")(self.table()[first:first + n].copy(), first, ramp)
        if ramp:
            self.pending.append((first, n))
        self.count()
        self.check()

    def refused(self):
        first, n = self.range(("inside", "span", "overlap")[int(self.rng.randint(3))])
        self.tape.refused(self.bad_table(first, n), first, bool(self.rng.randint(2)))
        self.count()
        self.check()

    def reset(self):
        self.tape.reset()
        self.pending, self.p = [], 0
        if self.plan == "resample":
            self.k = 0
        self.count()
        self.check()

    def delays(self, ranged):
        N, M = self.shape[2], self.shape[4]
        d = self.rng.randint(REVERB_MIN_DELAY, M + 1, (self.T, N)).astype(np.int32)
        if ranged:
            first, n = self.range(("inside", "span")[int(self.rng.randint(2))])
            self.tape.delays_tracks(d[first:first + n].copy(), first)
        else:
            self.tape.delays(d)
        self.count()
        self.check()

    def decay(self):
        self.tape.decay(float(self.rng.choice([0.25, 0.5, 0.75, 0.9375, 1.0])))
        self.count()
        self.check()

    def taps(self):
        self.hot = not self.hot
        K = self.shape[4]
        self.tape.taps(one_hot_taps(self.L, K) if self.hot else resample_taps32(self.shape[2], self.shape[3], K))
        self.count()
        self.check()

    # ---- the crossover's calls ----
    def ranged(self, kinds):
        """A range of two tracks or more of one of `kinds`."""
        for _ in range(20):
            first, n = self.range(kinds[int(self.rng.randint(len(kinds)))])
            if n >= 2:
                break
        return first, n

    def splits(self, kind=None):
        if kind is None:
            self.tape.splits(self.table())
        else:
            first, n = self.ranged((kind,))
            self.tape.splits_tracks(self.table()[first:first + n].copy(), first)
        self.count()
        self.check()

    def bad_rows(self, first, n):
        """Rows [first, first + n) of a good table with one value or one row the rule refuses, and a NaN behind it."""
        rng, S = self.rng, self.shape[2] - 1
        p = self.table()[first:first + n].copy()
        tiny = np.float32(-1e-30)
        spots = [(0, np.nan), (1, np.inf), (2, -np.inf), (0, 0.0), (0, 1.5), (0, tiny), (1, 1.0), (1, tiny), (2, 1.0),
                 (2, tiny), (0, "sum")]
        f, v = spots[int(rng.randint(len(spots)))]
        r, j = int(rng.randint(n)), int(rng.randint(S))
        p[r, j, f] = p[r, j, f] * np.float32(0.999) if isinstance(v, str) else v
        later = (r * S + j) * 3 + f + 1 + int(rng.randint(3 * S))
        if later < p.size:
            p.ravel()[later] = np.nan
        return p

    def splits_refused(self):
        first, n = self.ranged(("inside", "span"))
        self.tape.refused(self.bad_rows(first, n), first)
        self.count()
        self.check()

    def unset_run(self):
        self.tape.unset_run(self.block())
        self.count()
        self.check()

    # ---- the spectrum plan's calls ----
    def window(self):
        """A seeded positive window, a one-hot one and periodic Hann in turn (a new plan holds Hann)."""
        kind = ("positive", "one-hot", "hann")[self.windows % 3]
        self.windows += 1
        if kind == "positive":
            w = self.rng.uniform(0.1, 1.0, st.N).astype(np.float32)
        else:
            w = st.window_hann() if kind == "hann" else st.one_hot(int(self.rng.choice([0, 1, 511, 1023])))
        self.tape.window(w)
        self.count()
        self.check()

    def refused_window(self):
        """A value that is not finite (and another behind it), or a sum of zero."""
        rng = self.rng
        kind = int(rng.randint(4))
        if kind == 0:
            w = np.zeros(st.N, np.float32)
        elif kind == 1:
            w = np.where(np.arange(st.N) % 2 == 0, 1.0, -1.0).astype(np.float32)
        else:
            w = rng.uniform(0.1, 1.0, st.N).astype(np.float32)
            at = int(rng.randint(st.N))
            w[at] = w[min(at + 1 + int(rng.randint(8)), st.N - 1)] = (np.nan, np.inf, -np.inf)[int(rng.randint(3))]
        self.tape.refused_window(w)
        self.count()
        self.check()

    def good_edges(self):
        return sorted(int(v) for v in self.rng.choice(st.BINS + 1, self.shape[4] + 1, replace=False))

    def edges(self):
        self.tape.edges(self.good_edges())
        self.count()
        self.check()

    def refused_edges(self):
        e, rng = self.good_edges(), self.rng
        kind = int(rng.randint(4))
        if kind == 0:
            e[0] = -1
        elif kind == 1:
            e[-1] = st.BINS + 1
        else:
            b = 1 + int(rng.randint(len(e) - 1))
            e[b] = e[b - 1] - (kind == 3)                              # equal to the edge before it, or below it
        self.tape.refused_edges(e)
        self.count()
        self.check()

    def off_the_grid(self):
        """Runs until the position is no multiple of the hop."""
        while self.p % self.shape[2] == 0 and self.buffers < MAX_BUFFERS:
            self.run()

    def silent_batch(self):
        """Single buffers until three more end before the next frame does, then those three as one batch."""
        B, H = self.B, self.shape[2]
        self.cut()
        while self.p % H + 3 * B >= H and self.buffers < MAX_BUFFERS - 3:
            self.run()
            self.cut()
        self.runs(3, cuts=False)

    def steady(self):
        """No ramp pending behind this."""
        if self.pending:
            self.run()

    # ---- the scenes ----
    def scenes(self):
        rng, plan = self.rng, self.plan
        pick = lambda *v: v[int(rng.randint(len(v)))]                  # noqa: E731
        if plan in RAMPED:
            out = [
                # a ramped range, then an unramped range across part of it while that ramp is pending
                lambda: (self.steady(), self.set(True, pick("inside", "span")), self.set(False, "overlap"), self.runs(2)),
                # a refused set while a ramp is pending
                lambda: (self.set(True, pick(None, "span")), self.refused(), self.runs(2)),
                # a reset while a ramp is pending
                lambda: (self.set(True, pick(None, "inside", "span")), self.reset(), self.runs(1)),
                # two ramped sets between two batches; the second batch's first buffer ramps
                lambda: (self.runs(1), self.set(True), self.set(True, "overlap"), self.runs(3, cuts=False)),
                # a steady batch of three buffers or more
                lambda: (self.steady(), self.set(False), self.runs(3 + int(rng.randint(3)), cuts=False)),
                lambda: (self.steady(), self.reset(), self.runs(1)),
                lambda: (self.steady(), self.refused(), self.runs(1), self.cut(), self.runs(1)),
                lambda: (self.set(False, pick("inside", "span")), self.runs(1)),
            ]
            if plan == "reverb":
                out.append(lambda: (self.delays(False), self.runs(1), self.delays(True), self.runs(1)))
            if plan == "gate":                                         # holds run down across a cut: loud, then quiet
                out.append(lambda: (self.steady(), self.run(1.0), self.run(0.015625), self.cut(), self.run(0.015625)))
            if plan == "lim":                                          # a held minimum and a running release across a cut
                out.append(lambda: (self.steady(), self.run(4.0), self.cut(), self.run(0.015625), self.run(0.015625)))
            return out
        if plan == "xover":
            return [lambda: (self.runs(2, cuts=False), self.splits(), self.runs(2, cuts=False)),  # between two batches
                    # ranged sets between two buffers of what would have been one batch
                    lambda: (self.runs(1), self.splits("inside"), self.runs(1), self.splits("span"), self.runs(1)),
                    lambda: (self.splits_refused(), self.runs(1)),
                    lambda: (self.runs(1), self.reset(), self.runs(1)),
                    lambda: (self.cut(), self.runs(3 + int(rng.randint(3)), cuts=False))]
        if plan == "spec":
            B, H, bands = self.B, self.shape[2], self.shape[4]
            out = [lambda: (self.off_the_grid(), self.reset(), self.runs(2)),
                   lambda: (self.runs(2, cuts=False), self.window(), self.runs(2, cuts=False), self.window(),
                            self.runs(1), self.window(), self.runs(1)),
                   lambda: (self.refused_window(), self.runs(1)),
                   lambda: (self.cut(), self.runs(3 + int(rng.randint(2)), cuts=False))]
            if bands:
                out.append(lambda: (self.edges(), self.runs(1), self.refused_edges(), self.runs(1)))
            if 3 * B < H:
                out.append(self.silent_batch)
            if 2 * B >= 3 * H:                                         # two buffers hold three frames from any phase
                out.append(lambda: (self.cut(), self.runs(2 + int(rng.randint(2)), cuts=False)))
            return out
        if plan == "meter":
            return [lambda: (self.decay(), self.runs(3 + int(rng.randint(3)), cuts=False)),
                    lambda: (self.reset(), self.runs(2)),
                    lambda: (self.decay(), self.runs(1), self.cut(), self.runs(2)),
                    lambda: (self.runs(2), self.decay(), self.reset(), self.runs(1))]
        return [lambda: (self.reset(), self.runs(self.period + 2)),       # more buffers than a period behind a reset
                lambda: (self.taps(), self.runs(2), self.taps(), self.runs(2)),
                lambda: (self.runs(2), self.reset(), self.runs(1)),
                lambda: (self.cut(), self.runs(3, cuts=False))]

    def any_call(self):
        """One call of the plan's vocabulary."""
        rng, plan = self.rng, self.plan
        kinds = (None, "inside", "span", "overlap")
        if plan in RAMPED:
            menu = ["run"] * 3 + ["set", "set", "refused", "reset", "cut"] + (["delays"] if plan == "reverb" else [])
        elif plan == "meter":
            menu = ["run"] * 3 + ["decay", "reset", "cut"]
        elif plan == "xover":
            menu = ["run"] * 3 + ["splits", "splits", "splits_refused", "reset", "cut"]
        elif plan == "spec":
            menu = ["run"] * 3 + ["window", "refused_window", "reset", "cut"] + (["edges"] if self.shape[4] else [])
        else:
            menu = ["run"] * 3 + ["taps", "reset", "cut"]
        what = menu[int(rng.randint(len(menu)))]
        if what == "run":
            self.runs(1)
        elif what == "set":
            self.set(bool(rng.randint(2)), kinds[int(rng.randint(4))])
        elif what == "splits":
            self.splits(kinds[int(rng.randint(3))])
        elif what == "delays":
            self.delays(bool(rng.randint(2)))
        else:
            getattr(self, what)()

    def draw(self):
        scenes = self.scenes()
        if self.plan == "reverb":
            self.delays(False)
        if self.plan == "xover":                                       # the opening: a plan without rows
            self.unset_run(), self.splits_refused(), self.unset_run()
            self.splits(("inside", "span")[int(self.rng.randint(2))])
            self.runs(1)
        for i in self.rng.permutation(len(scenes)):
            scenes[int(i)]()
            if self.calls < self.steps and self.rng.randint(2):
                self.any_call()
        while self.calls < self.steps and self.buffers < MAX_BUFFERS:
            self.any_call()
        if self.tape.ops[-1][0] != "check":
            self.check()
        return self.tape


def freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, dict):
        for a in v.values():
            freeze(a)


@functools.lru_cache(maxsize=None)
def walk(plan, shape, seed, steps):
    """(the tape of calls, run()'s outputs per buffer, the carried state at the end, the host actor); read only."""
    d = Draw(plan, shape, seed, steps)
    tape = d.draw()
    for op in tape.ops:
        for a in op[1:]:
            freeze(a)
    for o in tape.outs:
        freeze(o)
    state = d.host.state()
    freeze(state)
    return tape.ops, tape.outs, state, d.host


def batches(ops):
    """The batches play(batch=True) makes of a tape: [(index of the first run op, buffers)]."""
    out, n, start, keyed = [], 0, None, None
    for i, op in enumerate(ops):
        if op[0] == "run" and n and keyed == (op[2] is not None):
            n += 1
            continue
        if n:
            out.append((start, n))
        n = 0
        if op[0] == "run":
            n, start, keyed = 1, i, op[2] is not None
    if n:
        out.append((start, n))
    return out


def census(w, ops):
    """What a tape holds, from the tape alone: a dict of counts and of the orderings the walks are for."""
    T = w.shape[0]
    c = collections.Counter(op[0] for op in ops)
    c.update("%s %s" % (op[0], "ramped" if op[-1] else "unramped") for op in ops if op[0] in SETS)
    heads = dict(batches(ops))
    period = HOSTS[w.plan](*w.shape).twin.period if w.plan == "resample" else None
    pending, k, since_reset, i_batch, seen_batch, ramp_since_batch = [], 0, 0, 0, False, False
    own, p = owner_tracks(w.plan, w.shape), 0
    if w.plan == "xover":
        names = [op[0] for op in ops if op[0] != "check"]
        c["the opening on a plan without rows"] = int(names[:5] == ["unset_run", "refused", "unset_run", "splits_tracks",
                                                                   "run"] and "splits" in names[5:])
    for i, op in enumerate(ops):
        name = op[0]
        if name.endswith("_tracks"):
            a, b = op[2], op[2] + op[1].shape[0]
            c["a ranged set across two owners"] += bool(a % own and b % own and a // own + 1 == (b - 1) // own)
            if w.plan == "lim":
                c["a range that starts or ends inside a link group"] += bool(a % w.shape[3] or b % w.shape[3])
        if name == "window":
            c["a %s window" % window_kind(op[1])] += 1
        if w.plan == "spec" and name == "reset":
            c["a reset off the hop grid"] += bool(p % w.shape[2])
            p = 0
        if w.plan == "spec" and name == "run":
            if i in heads:
                B, H = w.shape[1], w.shape[2]
                frames = st.count(p, heads[i] * B, H)
                c["a batch of three or more that emits no frame"] += heads[i] >= 3 and frames == 0
                c["a batch that emits more frames than buffers"] += heads[i] >= 2 and frames > heads[i]
            p += w.shape[1]
        if name in SETS or name == "refused":
            first, n = (op[2], op[1].shape[0]) if name != set_name(w.plan) else (0, T)
            others = [r for r in pending if r != (first, n) and r[0] < first + n and first < r[0] + r[1]]
            if name.endswith("_tracks") and others:
                c["a range set on another range's pending ramp"] += 1
                if not op[-1]:
                    c["an unramped range set on another range's pending ramp"] += 1
            if name == "refused" and pending:
                c["a refused set on a pending ramp"] += 1
            if name != "refused" and op[-1]:
                if pending:
                    c["two ramped sets before a buffer"] += 1
                if seen_batch:
                    ramp_since_batch = True
                pending.append((first, n))
        if name == "reset":
            c["a reset on a pending ramp"] += bool(pending)
            pending, k, since_reset = [], 0, 0
        if name == "run":
            if i in heads:
                i_batch = 0
                c["batches of %d" % heads[i]] += 1
                c["a batch whose first buffer ramps"] += bool(pending) and heads[i] >= 2
                c["a steady batch of three or more"] += (not pending) and heads[i] >= 3
                c["a ramp set between two batches"] += ramp_since_batch
                seen_batch, ramp_since_batch = True, False
            if period is not None:
                c["period - 1 -> 0 inside a batch"] += i_batch > 0 and k == 0 and since_reset > 0
                since_reset += 1
                c["buffers behind a reset, at most"] = max(c["buffers behind a reset, at most"], since_reset)
                k = (k + 1) % period
            i_batch += 1
            pending = []
    return dict(c)
