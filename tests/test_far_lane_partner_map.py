"""The far role's thread renaming and lane-half trades (conv_split_batch12_resident, k_conv_accel.hip), restated on the CPU.
A far group's physical thread p (wave fw = p >> 6, lane l = p & 63, j = l & 31) works as logical thread
    t = 32 fw + j            (l < 32)
    t = 256 - 32 fw - j      (l >= 32; fw = 0, j = 0: t = 128)
so that the holder of a thread's partner bins N - k, thread 256 - t, is lane l ^ 32 of the same wave and the partners'
values cross by v_permlane32_swap_b32 instead of two regions of the LDS image.  Threads 0 and 128 are their own partners."""
import numpy as np

N = 4096                # the far transform
NT = 256                # threads of a far group: logical thread t holds bins t + 256 r, r < 16 (register r)


def logical(p):
    fw, l = p >> 6, p & 63
    j = l & 31
    if l < 32:
        return 32 * fw + j
    return 128 if fw == 0 and j == 0 else 256 - 32 * fw - j


T_OF = np.array([logical(p) for p in range(NT)])
P_OF = np.argsort(T_OF)


def permlane32_swap(a, b):
    """v_permlane32_swap_b32 a, b: a's lanes 32-63 change places with b's lanes 0-31."""
    a, b = a.copy(), b.copy()
    hi, lo = a[32:].copy(), b[:32].copy()
    a[32:], b[:32] = lo, hi
    return a, b


def trade(a, b):
    """Two swaps on a register pair, (a, b) then (b, a)."""
    a, b = permlane32_swap(a, b)
    b, a = permlane32_swap(b, a)
    return a, b


def test_the_map_is_a_permutation():
    assert sorted(T_OF.tolist()) == list(range(NT))
    assert T_OF[0] == 0 and T_OF[32] == 128                            # the self-partner threads: lanes 0 and 32 of the first wave


def test_the_partner_is_the_other_half_of_the_same_wave():
    for p in range(NT):
        t = int(T_OF[p])
        if t in (0, 128):
            assert (256 - t) % 256 == t                               # its own partner
            continue
        assert P_OF[256 - t] == p ^ 32, (p, t)
    assert {int(T_OF[p]) for p in range(NT) if (256 - int(T_OF[p])) % 256 == int(T_OF[p])} == {0, 128}


def test_two_swaps_on_a_pair_give_the_partners_values_in_both_halves():
    x, y = np.arange(64), 100 + np.arange(64)
    a, b = trade(x, y)
    lanes = np.arange(64)
    assert np.array_equal(a, y[lanes ^ 32])                           # a holds the partner's b
    assert np.array_equal(b, x[lanes ^ 32])                           # b holds the partner's a


def partner_register(t, r):
    """(thread, register) that holds Z[N - k] for k = t + 256 r, r < 8: bin b lies in thread b % 256, register b // 256."""
    b = (N - (t + NT * r)) % N
    return b % NT, b // NT


def test_register_rule_of_each_class():
    for t in range(NT):
        for r in range(8):
            tt, rr = partner_register(t, r)
            if t == 0:
                assert (tt, rr) == (0, 0 if r == 0 else 16 - r)       # bin 0 with itself, bin 256 r with own register 16 - r
            elif t == 128:
                assert (tt, rr) == (128, 15 - r)                      # own register 15 - r
            else:
                assert (tt, rr) == (256 - t, 15 - r)                  # the partner's register 15 - r: its eight HIGH registers
    # thread 0's register 8 (bin N / 2) is nobody's partner
    assert all(partner_register(t, r) != (0, 8) for t in range(NT) for r in range(8))


def test_the_trades_as_the_kernel_issues_them():
    """Z trade: pairs (8 + i, 15 - i), i < 4, of the high registers give zp[i], zp[7 - i]; W trade: pairs (wp[i], wp[7 - i])
    land in registers 8 + i and 15 - i.  Tags (thread, register) through the swaps, wave by wave."""
    for fw in range(4):
        tl = T_OF[64 * fw: 64 * fw + 64]
        z = [NT * r + tl for r in range(16)]                          # register r of lane l: bin t + 256 r
        zp = [None] * 8
        for i in range(4):
            zp[i], zp[7 - i] = trade(z[8 + i], z[15 - i])
        for l in range(64):
            t = int(tl[l])
            if t in (0, 128):
                continue                                              # what these two receive is dropped
            for r in range(8):
                assert zp[r][l] == N - (t + NT * r), (fw, l, r)
        wp = [(N - (NT * r + tl)) % N for r in range(8)]              # wp[r]: the result for bin N - k
        hi = [None] * 16
        for i in range(4):
            hi[8 + i], hi[15 - i] = trade(wp[i], wp[7 - i])
        for l in range(64):
            t = int(tl[l])
            if t in (0, 128):
                continue
            for r in range(8, 16):
                assert hi[r][l] == t + NT * r, (fw, l, r)
    # own registers of the self-partner threads: thread 128's wp[r] is register 15 - r, thread 0's wp[r] register 16 - r
    for r in range(8):
        assert (N - (128 + NT * r)) == 128 + NT * (15 - r)
    for r in range(1, 8):
        assert (N - NT * r) == NT * (16 - r)


# ---- LDS bank conflicts of the renamed access patterns (entries of 8 bytes; positions as in the kernel) --------------------
# ds_write_b64: conflicts within groups of 16 contiguous lanes, bank = dword mod 32: entries must differ mod 16.
# ds_read_b64: within the two 32-lane halves, bank = dword mod 64: entries are compared mod 32.
def w0_of(t):
    return 17 * t


def rd_of(t):
    return t + (t >> 4)


def w1_of(t):
    b1 = (t >> 4) * 256 + (t & 15)
    return b1 + (b1 >> 4)


def worst(positions, group, modulus):
    """Largest number of DISTINCT entries on one bank pair within a lane group, over the groups of every wave."""
    out = 0
    for g0 in range(0, NT, group):
        pos = {int(x) for x in positions[g0:g0 + group]}               # the same entry twice is a broadcast, not a conflict
        out = max(out, int(np.bincount(np.array(sorted(pos)) % modulus, minlength=modulus).max()))
    return out


def doubled(positions, group, modulus):
    """Per lane group: how many bank pairs are hit by two distinct entries."""
    out = []
    for g0 in range(0, NT, group):
        pos = np.array(sorted({int(x) for x in positions[g0:g0 + group]}))
        out.append(int((np.bincount(pos % modulus, minlength=modulus) == 2).sum()))
    return out


def test_padded_writes_stay_conflict_free():
    ident = np.arange(NT)
    for tmap in (ident, T_OF):
        for r in range(16):
            assert worst(np.array([w0_of(int(t)) + r for t in tmap]), 16, 16) == 1          # pass-0 writes
            assert worst(np.array([w1_of(int(t)) + 17 * r for t in tmap]), 16, 16) == 1     # pass-1 writes


def test_padded_reads_keep_their_one_two_way_bank():
    ident = np.arange(NT)
    for r in range(16):
        for tmap in (ident, T_OF):
            pos = np.array([rd_of(int(t)) + 272 * r for t in tmap])
            assert worst(pos, 32, 32) == 2
            assert doubled(pos, 32, 32) == [1] * 8                    # one bank pair with two entries per half, as before the renaming


def test_middle_pass_twiddle_rows_are_read_as_before():
    # tw1 + 15 (t & 15) + r: a half of 32 lanes asks for the same sixteen rows under either naming (equal entries: one fetch)
    for g0 in range(0, NT, 32):
        assert {int(t) & 15 for t in T_OF[g0:g0 + 32]} == set(range(16))


def test_every_half_is_a_run_of_consecutive_threads():
    for g0 in range(0, NT, 32):
        ts = sorted(int(t) for t in T_OF[g0:g0 + 32])
        if g0 == 32:                                                  # the first wave's upper half: 128 and 225 .. 255
            assert ts == [128] + list(range(225, 256))
        else:
            assert ts == list(range(ts[0], ts[0] + 32))
            assert ts[0] % 32 == (0 if (g0 & 32) == 0 else 1)         # the upper halves' runs are one off a multiple of 32
