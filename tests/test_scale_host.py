"""The conditions tests/test_scale_gpu.py rests on, from shapes and a numpy model alone (no GPU).

  * Every case of the boundary tier passes the boundaries it claims: the tensors it names (the call's largest, and every
    other tensor of that reach) have exactly one buffer across each of 2^30, 2^31 and 2^32 elements and one whole buffer
    at least above it; every other tensor that grows with n is held to the boundaries its size reaches, and the input
    of every call passes 2^30 and 2^31 at least.
  * A wrapped offset is seen.  For an element index computed as int32, as uint32, and a byte offset computed as
    uint32, every buffer that straddles or lies above the defect's boundary lands in front of the tensor (an access
    outside it) or in ANOTHER buffer of the fill, whose contents differ: the comparison of plan A with plan B is not a
    comparison of a buffer with itself.  The same defects in a scaled-down model (12-bit offsets) make oracle (1) differ
    on exactly those buffers, or fault.
  * The shard of oracle (2) ends in a partial owner for every plan at 65 539 tracks, and its pieces are aligned to every
    plan's owner and link group.
"""
import numpy as np
import pytest

import scale_helpers as sh

EDGE = sh.edge_cases()
BENCH = sh.bench_cases()


def ids(cases):
    return [sh.case_id(c) for c in cases]


def test_the_default_boundary_shape_is_the_one_the_table_states():
    u = sh.EDGE_T * sh.EDGE_B
    assert u == 67111936
    assert [sh.straddler(u, b) for b in sh.BOUNDARIES] == [15, 31, 63]
    assert sh.n_for(u) == 65                        # 63 across, 64 whole above; the in-place plans run 66 = two above
    for own in (64, 32, 16, 8, 4):
        assert sh.EDGE_T % own == 3
    assert sh.EDGE_T % 2 == 1
    assert 4 * (1 << 30) == 1 << 32                 # 2^30 elements: the byte offset 2^32


@pytest.mark.parametrize("c", EDGE, ids=ids(EDGE))
def test_a_boundary_case_has_a_buffer_across_and_a_buffer_above_every_boundary_it_claims(c):
    t = sh.tensors(c)
    names = sh.named(c)
    assert names and max(t, key=t.get) in names
    for name, unit in t.items():
        claimed = list(sh.BOUNDARIES) if name in names else sh.reached(unit, c.n)
        for b in claimed:
            across = [k for k in range(c.n) if k * unit < b < (k + 1) * unit]
            above = [k for k in range(c.n) if k * unit >= b]
            assert len(across) == 1 and across[0] == sh.straddler(unit, b), (name, b)
            assert len(above) >= 1, (name, b)
            assert (b % unit) != 0                   # no buffer ends on the boundary: the one across is really across
    big = [name for name in t if name in ("in", "io", "rows")]
    assert big and all(set(sh.reached(t[name], c.n)) >= {1 << 30, 1 << 31} for name in big)
    assert sh.need_bytes(c) < 64 << 30


def test_the_boundary_cases_are_the_smallest_that_pass():
    """The default shape runs 66 buffers (two whole buffers above 2^32 elements); a call with a tensor larger than its
    input runs what that tensor needs and no more."""
    for c in EDGE:
        largest = max(sh.tensors(c).values())
        if largest == c.T * c.B:
            assert c.n == 66
        else:
            assert c.n == sh.n_for(largest) and sh.reached(largest, c.n - 1) != list(sh.BOUNDARIES)


@pytest.mark.parametrize("c", BENCH + [sh.SPEC_LIMIT], ids=ids(BENCH + [sh.SPEC_LIMIT]))
def test_a_bench_case_is_the_bench_shape(c):
    t = sh.tensors(c)
    if c is sh.SPEC_LIMIT:
        assert c.n * t["in"] == 1 << 31 and c.n * sh.frames_per_buffer(c) * ((c.T // 2 + 3) // 4) == 1 << 23
    else:
        assert (c.T, c.B, c.n) == (8192, 512, 32) and c.n * max(t.values()) < 1 << 30
    assert sh.need_bytes(c) < 64 << 30


@pytest.mark.parametrize("defect", sh.DEFECTS)
@pytest.mark.parametrize("c", EDGE, ids=ids(EDGE))
def test_a_wrapped_offset_lands_outside_the_tensor_or_in_another_buffer(c, defect):
    first = {"int32 element index": 1 << 31, "uint32 element index": 1 << 32, "uint32 byte offset": 1 << 30}[defect]
    for name in sh.named(c):
        unit = sh.tensors(c)[name]
        wrapped = sh.wrapped_buffers(unit, c.n, defect)
        assert sorted(wrapped) == list(range(sh.straddler(unit, first), c.n)), (name, defect)
        for b, lands in wrapped.items():
            for e, land in zip((0, unit - 1), lands):
                # the buffer across the boundary starts below it: its first element is where it belongs
                if b == sh.straddler(unit, first) and e == 0:
                    assert land == (b, 0)
                    continue
                assert land is None or land[0] != b, (name, defect, b)
            assert any(land is None or land[0] != b for land in lands)


def test_two_blocks_of_the_fill_differ():
    import torch
    a, b, a2 = (torch.empty(130, 96) for _ in range(3))
    lv = sh.levels(130, "cpu")[:, None]
    sh.fill(a, 7, 15, lv)
    sh.fill(b, 7, 63, lv)
    sh.fill(a2, 7, 15, lv)
    assert sh.same_bits(a, a2) and not sh.same_bits(a, b)
    assert torch.isfinite(a).all() and float(a.abs().max()) <= 1.0
    assert float((sh.as_words(a) != sh.as_words(b)).float().mean()) > 0.99
    assert float(a[5].abs().max()) <= 1.0 and float(a[4].abs().max()) <= 2.0 ** -4      # a level per track
    k = torch.empty(130, 96)
    sh.fill(k, 8, 15, lv)                           # another seed: a key is not the input
    assert float((sh.as_words(a) != sh.as_words(k)).float().mean()) > 0.99


def test_the_comparison_is_of_bits():
    import torch
    nan = torch.tensor([float("nan"), 0.0, 1.0])
    assert sh.same_bits(nan, nan.clone())
    assert not sh.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    other = nan.clone().view(torch.int32)
    other[0] += 1                                   # another NaN
    assert not sh.same_bits(nan, other.view(torch.float32))


@pytest.mark.parametrize("defect", sh.DEFECTS)
def test_oracle_one_fails_on_the_modelled_wrap(defect):
    """The boundary shapes scaled down: offsets of 12 bits, buffers of 67 elements (2^10, 2^11 and 2^12 fall inside a
    buffer each), n as n_for picks it.  The exact model passes; the defective one differs on every buffer from the one
    across its boundary on, or faults, which on the device is an access outside the tensor."""
    bits, unit = 12, 67
    n = sh.n_for(unit, 1 << bits)
    x = np.random.RandomState(3).uniform(-1, 1, n * unit).astype(np.float32)
    assert sh.model_differing(x, unit, None, bits) == []
    first = {"int32 element index": 1 << (bits - 1), "uint32 element index": 1 << bits,
             "uint32 byte offset": 1 << (bits - 2)}[defect]
    want = list(range(sh.straddler(unit, first), n))
    assert sorted(sh.wrapped_buffers(unit, n, defect, bits)) == want
    try:
        got = sh.model_differing(x, unit, defect, bits)
    except IndexError:
        assert defect == "int32 element index"      # a negative index: in front of the tensor
        return
    assert got == want and len(want) >= 2


@pytest.mark.parametrize("c", EDGE, ids=ids(EDGE))
def test_the_shard_ends_in_a_partial_owner(c):
    sel = sh.shard_tracks(c.T)
    own = sh.owner_tracks(c)
    last = sel[2 * sh.CHUNK:]
    assert len(sel) == 2 * sh.CHUNK + 3 and last.tolist() == [c.T - 3, c.T - 2, c.T - 1]
    assert sel[0] == 0 and sh.CHUNK < sel[sh.CHUNK] < c.T - 2 * sh.CHUNK and sel[sh.CHUNK] % sh.CHUNK == 0
    if own is None:
        assert c.plan == "mix"                      # no shard: a bus sums every track
        return
    assert sh.CHUNK % own == 0 and last[0] % own == 0 and len(last) % own != 0
    assert dict(c.opts).get("link", 1) == 1         # 65 539 is odd


@pytest.mark.parametrize("c", BENCH, ids=ids(BENCH))
def test_the_bench_shard_is_aligned_to_owners_and_link_groups(c):
    sel = sh.shard_tracks(c.T)
    own, link = sh.owner_tracks(c), dict(c.opts).get("link", 1)
    assert len(sel) == 3 * sh.CHUNK and sel[-1] == c.T - 1          # 8 192 tracks end on an owner: no partial one here
    assert own is None or sh.CHUNK % own == 0
    assert sh.CHUNK % link == 0 and c.T % link == 0
