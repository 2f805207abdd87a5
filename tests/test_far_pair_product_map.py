"""The far role's spectral product by bin pairs (conv_split_batch12_resident, k_conv_accel.hip), restated on the CPU: which
thread forms which bin from which entry of the spectra on which branch, and which thread writes and reads which position of
the two exchange regions of a group's LDS image in which barrier interval.  Checked against the rule of load_spectra /
spectral_product for the thread that holds the bin after forward pass 2 (thread b mod 256 holds bin b)."""
import numpy as np

N = 4096                # the far transform
NT = 256                # threads of a far group: thread t holds bins t + 256 r, r < 16
HALF = N // 2           # entries of one exchange region; the spectra have HALF + 1 entries

# barrier intervals of a transform, counted from its first: 1-6 the first period, 7-12 the second
Z_WRITE, Z_READ, W_WRITE, W_READ = 5, 6, 6, 7


def owner_rule(b):
    """(spectra index, conjugate branch) of bin b by load_spectra_part / spectral_product_part in the thread that holds it."""
    t, r = b % NT, b // NT
    if r < 8:
        return b, False
    if r > 8 or t != 0:
        return N - b, True
    return b, False                      # bin N / 2, thread 0


def products(t):
    """What thread t forms: [(bin, spectra index, conjugate branch, Z operand bin, partner operand bin)]."""
    out = []
    for r in range(8):
        k = t + NT * r
        out.append((k, k, False, k, (N - k) % N))                     # W[k] = cfma_cj(Z[N - k], M, cmul(Z[k], P))
        if k == 0:
            out.append((HALF, HALF, False, HALF, HALF))              # thread 0: bin N / 2 where bin 0's partner would stand
        else:
            out.append((N - k, k, True, N - k, k))                   # W[N - k] = cfma_cjcj(Z[k], M, cmulc(Z[N - k], P))
    return out


def z_writes(t):
    """Region 0, interval Z_WRITE: (position, bin whose Z is stored)."""
    return [(t + NT * (r - 8), t + NT * r) for r in range(8, 16)]


def z_reads(t):
    """Region 0, interval Z_READ: (position, bin whose Z the reader uses from it, or None: thread 0 takes Z[0] from its registers)."""
    return [((HALF - t - NT * r) % HALF, None if t + NT * r == 0 else N - (t + NT * r)) for r in range(8)]


def w_writes(t):
    """Region 1, interval W_WRITE: (position, bin whose W is stored)."""
    return [((HALF - t - NT * r) % HALF, HALF if t + NT * r == 0 else N - (t + NT * r)) for r in range(8)]


def w_reads(t):
    """Region 1, interval W_READ: (position, bin the reader takes it for)."""
    return [(t + NT * (r - 8), t + NT * r) for r in range(8, 16)]


def test_every_bin_is_formed_once():
    bins = np.array([p[0] for t in range(NT) for p in products(t)])
    assert bins.size == N
    assert np.array_equal(np.sort(bins), np.arange(N))


def test_every_bin_gets_its_owners_entry_branch_and_operands():
    for t in range(NT):
        for b, idx, conj, zb, pb in products(t):
            assert (idx, conj) == owner_rule(b), (t, b)
            assert 0 <= idx <= HALF
            assert zb == b and pb == (N - b) % N, (t, b)             # z = Z[b], zraw = Z[(N - b) mod N], as in the owner's call


def test_one_fetch_per_entry_of_the_spectra():
    idx = np.array([t + NT * r for t in range(NT) for r in range(8)] + [HALF])     # the eight low bins; thread 0: and N / 2
    assert np.array_equal(np.sort(idx), np.arange(HALF + 1))
    for t in range(NT):
        fetched = {t + NT * r for r in range(8)} | ({HALF} if t == 0 else set())
        assert {p[1] for p in products(t)} == fetched


def test_each_region_position_is_written_once_and_read_once_with_the_value_the_reader_wants():
    for writes, reads in ((z_writes, z_reads), (w_writes, w_reads)):
        held = {}
        for t in range(NT):
            for pos, b in writes(t):
                assert 0 <= pos < HALF and pos not in held
                held[pos] = b
        assert sorted(held) == list(range(HALF))
        seen = set()
        for t in range(NT):
            for pos, b in reads(t):
                assert 0 <= pos < HALF and pos not in seen
                seen.add(pos)
                if b is not None:
                    assert held[pos] == b, (t, pos)
        assert len(seen) == HALF


def test_no_region_is_written_in_the_interval_in_which_it_is_read():
    assert Z_WRITE < Z_READ and W_WRITE < W_READ                       # a barrier between a region's writes and its reads
    assert Z_READ == W_WRITE                                           # the one interval with reads and writes: in different regions
    # the padded layout of the next exchange (inverse pass 0's write, the whole image) comes behind the barrier that ends W_READ
    assert W_READ + 1 == 8


def test_the_reader_of_every_high_result_is_the_thread_that_holds_the_bin():
    for t in range(NT):
        assert [b for _, b in w_reads(t)] == [t + NT * r for r in range(8, 16)]
        low = [p[0] for p in products(t) if p[0] < HALF]
        assert low == [t + NT * r for r in range(8)]                  # the low results never leave the thread


def test_thread_0():
    p = products(0)
    assert p[0] == (0, 0, False, 0, 0)                                 # bin 0: its own partner, formed once
    assert p[1] == (HALF, HALF, False, HALF, HALF)                     # bin N / 2: thread 0's own, pm[N / 2], not conjugated
    assert sum(1 for q in p if q[0] == 0) == 1
    for r in range(1, 8):                                              # its other high bins: partners of its own low bins
        assert (N - NT * r, NT * r, True, N - NT * r, NT * r) in p
    assert z_reads(0)[0] == (0, None)                                  # the wrapped position: read, not used
    assert w_writes(0)[0] == (0, HALF) and w_reads(0)[0] == (0, HALF)  # bin N / 2 through position 0 of the second region
    assert dict(z_writes(0))[0] == HALF
    for r in range(1, 8):                                              # written and read by thread 0 itself, no branch
        assert ((HALF - NT * r), N - NT * r) in z_writes(0) and ((HALF - NT * r), N - NT * r) in z_reads(0)
