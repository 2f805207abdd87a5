"""What the scale suite shares (tests/test_scale_host.py on the CPU, tests/test_scale_gpu.py on the device).  A plain
module like plan_helpers.py.

The suite holds the thirteen track plans where no host twin runs: at the shapes of tools/*_bench.py and where a tensor
of one call passes 2^30, 2^31 and 2^32 elements.  Its reference is the contract itself, two properties that the small
suites assert bit for bit:

  (1) a batch is its per-buffer calls: plan A makes one process_batch over [n][...], plan B n process calls on a
      scratch block each.  B's pointers are advanced on the host, so inside B's kernels every offset stays below one
      buffer; an offset that wraps inside A's kernel reads or writes another buffer, and A then differs from B on the
      buffers that straddle or lie above the boundary.
  (2) a shard aligned to owners is the whole plan's tracks: plan C holds three pieces of CHUNK tracks (the first, one
      in the middle, the last, which is partial at 65 539 tracks) and must give B's bits on them.  C has the size of
      plan that the small suites tie to the host twins.

Here: the cases, the arithmetic that picks their shapes, the seeded fill, the comparison of bits, and a model of a
wrapped offset that the host test uses to show that (1) sees it."""
import collections

import numpy as np

BOUNDARIES = (1 << 30, 1 << 31, 1 << 32)          # elements; 2^30 floats are 2^32 bytes
CHUNK = 64                  # tracks of a piece of the shard: a multiple of every plan's owner (64, 32, 16, 8, 4, a pair)
BENCH_T, BENCH_B, BENCH_N = 8192, 512, 32         # tools/*_bench.py: 8 192 tracks of 512 samples, a batch of 32
EDGE_T, EDGE_B = 65539, 1024                      # 65 539 = 1024 x 64 + 3: three tracks in the last owner, one in the last pair
EDGE_N = 66                                       # one buffer is 67 111 936 floats: 66 of them are 16.5 GiB
BINS = 513
RAMPED = ("mix", "delay", "dyn", "reverb", "gate", "lim")           # the plans with a ramped table
DEFECTS = ("int32 element index", "uint32 element index", "uint32 byte offset")

Case = collections.namedtuple("Case", "plan opts T B n")            # opts: a sorted tuple of (name, value)


def case(plan, T, B, n, **opts):
    return Case(plan, tuple(sorted(opts.items())), T, B, n)


def case_id(c):
    return "-".join([c.plan] + ["%s%s" % kv for kv in c.opts] + ["%dx%dx%d" % (c.T, c.B, c.n), "%.1fGiB" % (need_bytes(c) / 2.0 ** 30)])


def owner_tracks(c):
    """Tracks of the plan's smallest owner (a wave or a workgroup that carries them together): what a shard must be
    aligned to.  eq: the scan's wave owns a track, the ordered kernel's workgroup 64; delay: a wave a track, a workgroup
    four; reverb: 64 / lines; gate: a wave 16; crossover: 64 / G (G = 1, 2, 4 lanes a track for 2, 3, 4 bands); limiter:
    8; the STFT plans: a pair.  The mix plan has no owner: a bus sums every track."""
    o = dict(c.opts)
    if c.plan == "reverb":
        return 64 // o["lines"]
    if c.plan == "xover":
        return 64 >> (o["bands"] - 2)
    return {"eq": 64, "eqseq": 64, "delay": 4, "meter": 64, "resample": 64, "dyn": 64, "gate": 16, "lim": 8,
            "spec": 2, "resyn": 2, "dn": 2, "dnrows": 2, "mix": None}[c.plan]


def shard_tracks(T):
    """The tracks of plan C: the first CHUNK, the CHUNK in the middle, and the last piece, T - CHUNK (pieces - 1)."""
    pieces = -(-T // CHUNK)
    assert pieces >= 3
    picked = [0, pieces // 2, pieces - 1]
    return np.concatenate([np.arange(p * CHUNK, min((p + 1) * CHUNK, T)) for p in picked])


def frames_per_buffer(c):
    o = dict(c.opts)
    assert c.B % o["hop"] == 0                     # the frame count of a buffer is then the same for every buffer
    return c.B // o["hop"]


def tensors(c):
    """name -> elements per buffer (per frame for the rows form of denoise) of every tensor of the call that grows with
    n, in the call's order.  "io": the header allows d_out == d_in and the case runs in place."""
    o, u, T, B = dict(c.opts), c.T * c.B, c.T, c.B
    p = c.plan
    if p in ("eq", "eqseq", "delay"):
        return {"io": u}
    if p in ("dyn", "gate"):
        t = {"io": u}
        if o.get("keyed"):
            t["key"] = u
        t["gr" if p == "dyn" else "act"] = T
        return t
    if p == "lim":
        return {"io": u, "gr": T}
    if p == "reverb":
        return {"io": u} if o["outs"] == 1 else {"in": u, "out": o["outs"] * u}
    if p == "mix":
        return {"in": u, "out": o["buses"] * B}
    if p == "meter":
        return {"in": u, "fields": 8 * T}
    if p == "resample":
        g = np.gcd(o["up"], o["down"])
        return {"in": u, "out": T * int(-(-(B * (o["up"] // g)) // (o["down"] // g)))}
    if p == "xover":
        return {"in": u, "out": o["bands"] * u}
    if p == "spec":
        width = 2 * BINS if o["mode"] == "complex" else (o["bands"] or BINS)
        return {"in": u, "rows": frames_per_buffer(c) * T * width}
    if p == "resyn":
        return {"rows": frames_per_buffer(c) * T * 2 * BINS, "out": u}
    if p == "dn":
        return {"in": u, "out": u}
    assert p == "dnrows"
    return {"io": T * 2 * BINS}


def state_bytes(c):
    """Bytes of one plan's carried state, from above: the rings of the delay (a power of two >= max_delay + 3 + B floats
    a track) and of the reverb (>= max_delay + 64 a line); 16 KiB a track covers every other plan (the denoise plan's
    history, accumulator, mask and thresholds are 14 KiB)."""
    o = dict(c.opts)
    pow2 = lambda v: 1 << (int(v) - 1).bit_length()                  # noqa: E731
    if c.plan == "delay":
        return 4 * c.T * pow2(o["max_delay"] + 3 + c.B)
    if c.plan == "reverb":
        return 4 * c.T * o["lines"] * pow2(o["max_delay"] + 64)
    return c.T << 14


def need_bytes(c):
    """Device bytes of a case, from above: every tensor of plan A's call at full size, four scratch blocks of the
    largest buffer (B's input, key and output, and a comparison's temporary), the state of plans A and B and the copy
    of each that state() makes, and 1 GiB for the tables, the shard and the allocator's slack."""
    t = tensors(c)
    return 4 * (c.n * sum(t.values()) + 4 * max(t.values())) + 4 * state_bytes(c) + (1 << 30)


# ---- the arithmetic that picks shapes ----
def straddler(unit, boundary):
    """The buffer of `unit` elements that holds elements on both sides of `boundary`; None: a buffer ends exactly there."""
    q, r = divmod(boundary, unit)
    return q if r else None


def n_for(unit, boundary=BOUNDARIES[-1]):
    """The smallest n with one buffer across `boundary` and one whole buffer above it."""
    assert straddler(unit, boundary) is not None
    return boundary // unit + 2


def reached(unit, n):
    """The boundaries that n buffers of `unit` elements straddle once and lie above with one whole buffer at least."""
    return [b for b in BOUNDARIES if straddler(unit, b) is not None and n >= n_for(unit, b)]


def edge_case(plan, **opts):
    """A case of the boundary tier.  The default shape, where no tensor is larger than the input [n][T][B], takes n = 66:
    buffer 63 across 2^32 elements, 64 and 65 above.  A call with a larger tensor takes the smallest n that puts one
    whole buffer of THAT tensor above 2^32 elements."""
    probe = case(plan, EDGE_T, EDGE_B, 1, **opts)
    largest = max(tensors(probe).values())
    return probe._replace(n=EDGE_N if largest == EDGE_T * EDGE_B else n_for(largest))


def named(c):
    """The tensors of a boundary case that pass all three boundaries (the largest, and every other of that reach)."""
    return [k for k, u in tensors(c).items() if reached(u, c.n) == list(BOUNDARIES)]


# ---- the cases ----
def bench_cases():
    """The settings of tools/*_bench.py at 8 192 tracks x 512 samples, a batch of 32; below every boundary."""
    def c(plan, **o):
        return case(plan, BENCH_T, BENCH_B, BENCH_N, **o)
    out = [c(p, sections=s) for p in ("eq", "eqseq") for s in (1, 8)]
    out += [c("mix", buses=m, layout=l) for m in (2, 64) for l in ("track", "sample")]
    out += [c("delay", interp=i, max_delay=1024) for i in ("linear", "lagrange3")]
    out += [c("meter", window=w) for w in (1, 38)]
    out += [c("resample", up=u, down=d, taps=k) for u, d, k in ((160, 147, 32), (147, 160, 40), (2, 1, 32))]
    out += [c("dyn", keyed=k, link=l) for k in (False, True) for l in (1, 2)]
    out += [c("reverb", lines=8, outs=2, max_delay=4096)]
    out += [c("gate", keyed=k, link=1) for k in (False, True)]
    out += [c("xover", bands=k) for k in (2, 3, 4)]
    out += [c("lim", lookahead=64, link=l) for l in (1, 64)]
    out += [c("spec", hop=h, mode=m, bands=b) for h in (256, 512) for m, b in (("complex", 0), ("power", 0), ("power", 31))]
    out += [c("resyn", hop=h) for h in (256, 512)]
    out += [c(p, hop=h) for h in (256, 512) for p in ("dn", "dnrows")]
    return out


def edge_cases():
    """The boundary tier: 65 539 tracks x 1 024 samples, every plan at its cheapest setting; hop 1 024, so that a buffer
    of an STFT plan is a frame.  The table (buffers, and what a call of plan A holds on the device):

        plan        tensor(s) past 2^32 elements          n    bytes
        eq, eqseq   [n][T][B] in place                    66   16.5 GiB
        delay, dyn, gate, lim, reverb (1 output): the same
        mix         in [n][T][B]                          66   16.5 GiB   (out [n][1][B] is small)
        meter       in [n][T][B]                          66   16.5 GiB   (rows [n][T][8] are small)
        resample    out [n][T][2 B] (1 -> 2)              33   16.5 GiB + in 8.3 GiB (in passes 2^30 and 2^31)
        xover       out [n][2][T][B]                      33   16.5 GiB + in 8.3 GiB (in passes 2^30 and 2^31)
        spec        rows [F][T][513][2], in [n][T][B]     65   16.3 GiB + 16.3 GiB
        resyn       rows [F][T][513][2], out [n][T][B]    65   16.3 GiB + 16.3 GiB
        dn          in, out [n][T][B] (no overlap)        66   16.5 GiB + 16.5 GiB
        dnrows      rows [F][T][513][2] in place          65   16.3 GiB

    Out of scope: one buffer of 2^31 elements or more (T x B); no bench or user shape is near it."""
    e = edge_case
    return [e("eq", sections=1), e("eqseq", sections=1), e("mix", buses=1, layout="track"),
            e("delay", interp="linear", max_delay=16), e("meter", window=1), e("resample", up=2, down=1, taps=4),
            e("dyn", keyed=False, link=1), e("reverb", lines=4, outs=1, max_delay=64), e("gate", keyed=False, link=1),
            e("xover", bands=2), e("lim", lookahead=4, link=1), e("spec", hop=1024, mode="complex", bands=0),
            e("resyn", hop=1024), e("dn", hop=1024), e("dnrows", hop=1024)]


# the largest call the spectrum plan accepts: frames x groups = 1024 x 8192 = 2^23 workgroups, 2^31 threads, and an
# input of exactly 2^31 elements
SPEC_LIMIT = case("spec", 65536, 1024, 32, hop=32, mode="power", bands=1)


# ---- the seeded fill ----
def levels(T, device):
    """A level per track: 1, 1/2, 1/4, 1/8, 1/16 in turn."""
    import torch
    return torch.tensor([2.0 ** -(t % 5) for t in range(5)], dtype=torch.float32, device=device).repeat(-(-T // 5))[:T]


def fill(dst, seed, index, level=None):
    """Block `index` of fill `seed` into dst (any device, float32, contiguous): uniform noise in [-1, 1), finite
    everywhere, times `level` (a tensor that broadcasts against dst).  The values depend on (seed, index), dst's shape
    and its device alone, so a block can be made again where it is needed."""
    import torch
    g = torch.Generator(device=dst.device)
    g.manual_seed((int(seed) << 24) + int(index))
    dst.uniform_(-1.0, 1.0, generator=g)
    if level is not None:
        dst.mul_(level)
    return dst


# ---- the comparison ----
def as_words(t):
    import torch
    return t.contiguous().view(-1).view(torch.int32)


def differs(a, b):
    """A device flag (no synchronisation): do a and b differ in any bit?  On integer views: two NaNs of the same bits
    are the same, +0 and -0 are not."""
    a, b = as_words(a), as_words(b)
    assert a.numel() == b.numel()
    return (a != b).any()


def same_bits(a, b):
    return not bool(differs(a, b))


# ---- a wrapped offset ----
def aliased(e, defect, bits=32):
    """Where element index e (exact) lands when `defect` computes it in `bits` bits: an int (negative: in front of the
    tensor)."""
    m = 1 << bits
    if defect == "int32 element index":
        return (e + m // 2) % m - m // 2
    if defect == "uint32 element index":
        return e % m
    assert defect == "uint32 byte offset"
    return ((4 * e) % m) // 4


def wrapped_buffers(unit, n, defect, bits=32):
    """The buffers of [n][unit] that an access through `defect` takes from or puts somewhere else: {buffer: where its
    first and last element land, as (buffer, element) or None outside the tensor}; empty if nothing wraps."""
    out = {}
    for b in range(n):
        lands = []
        for e in (b * unit, (b + 1) * unit - 1):
            a = aliased(e, defect, bits)
            lands.append(None if not 0 <= a < n * unit else divmod(a, unit))
        if lands != [(b, 0), (b, unit - 1)]:
            out[b] = lands
    return out


def model_batch(x, unit, defect, bits):
    """The model of plan A with `defect` in its READ offset, in numpy: out[b][i] = 2 x[wrapped(b unit + i)] over
    x [n unit]; an index outside x raises IndexError, the model's fault.  defect None: the exact kernel, and plan B."""
    e = np.arange(x.size, dtype=np.int64)
    if defect is not None:
        e = np.array([aliased(int(v), defect, bits) for v in e], np.int64)
    if (e < 0).any() or (e >= x.size).any():
        raise IndexError("%s: an access outside the tensor" % defect)
    return np.float32(2.0) * x[e]


def model_differing(x, unit, defect, bits):
    """Oracle (1) on the model: the buffers on which the defective batch differs from per-buffer calls."""
    n = x.size // unit
    a = model_batch(x, unit, defect, bits).view(np.uint32).reshape(n, unit)
    b = np.stack([model_batch(x[i * unit:(i + 1) * unit], unit, None, bits) for i in range(n)]).view(np.uint32)
    return [i for i in range(n) if not np.array_equal(a[i], b[i])]
