"""The first exchange of the wave-held 1024-point transform (gab_fft.hpp, WaveFFT1024) as lane-half swaps: the map, on the
host.  Pass 0 leaves output k0 of butterfly lane + 64 m in register m + 4 k0, which is y[4 lane + 256 m + k0]; pass 1 wants
v'[r'] = y[L' + 64 r'].  Two swap stages with the instructions' semantics must leave, in PHYSICAL lane p and register
m + 4 k, the entry y[L'(p) + 64 (4 m + k)] with L'(p) = 4 (p & 15) + (p >> 4)."""
import numpy as np


def permlane32_swap(a, b):
    """v_permlane32_swap_b32 a, b: a's lanes 32-63 change places with b's lanes 0-31."""
    a, b = a.copy(), b.copy()
    hi, lo = a[32:].copy(), b[:32].copy()
    a[32:], b[:32] = lo, hi
    return a, b


def permlane16_swap(a, b):
    """v_permlane16_swap_b32 a, b: a's odd 16-lane rows change places with b's even rows (row 1 with row 0, 3 with 2)."""
    a, b = a.copy(), b.copy()
    for row in (0, 2):
        odd, even = a[16 * (row + 1):16 * (row + 2)].copy(), b[16 * row:16 * (row + 1)].copy()
        a[16 * (row + 1):16 * (row + 2)], b[16 * row:16 * (row + 1)] = even, odd
    return a, b


def virtual_lane(p):
    return 4 * (p & 15) + (p >> 4)


def after_pass0():
    """tag[lane, reg] = the y position held there after pass 0."""
    tag = np.empty((64, 16), np.int64)
    for lane in range(64):
        for m in range(4):
            for k0 in range(4):
                tag[lane, m + 4 * k0] = 4 * lane + 256 * m + k0
    return tag


def swapped(tag):
    v = [tag[:, r] for r in range(16)]
    for m in range(4):                                        # register bit 3 (k0 bit 1) against lane bit 5
        v[m], v[m + 8] = permlane32_swap(v[m], v[m + 8])
        v[m + 4], v[m + 12] = permlane32_swap(v[m + 4], v[m + 12])
    for m in range(4):                                        # register bit 2 (k0 bit 0) against lane bit 4
        v[m], v[m + 4] = permlane16_swap(v[m], v[m + 4])
        v[m + 8], v[m + 12] = permlane16_swap(v[m + 8], v[m + 12])
    return np.stack(v, axis=1)


def test_two_swap_stages_are_the_first_exchange():
    tag = after_pass0()
    assert sorted(tag.ravel().tolist()) == list(range(1024))
    got = swapped(tag)
    for p in range(64):
        for m in range(4):
            for k in range(4):
                assert got[p, m + 4 * k] == virtual_lane(p) + 64 * (4 * m + k), (p, m, k)


def test_the_virtual_lane_is_a_permutation():
    assert sorted(virtual_lane(p) for p in range(64)) == list(range(64))


def test_pass1_names_under_the_virtual_lane():
    """What pass 1 takes from its lane number, said with the physical lane: the twiddle base W64^(L' & 3) is W64^(p >> 4);
    its outputs go to row L' >> 2 = p & 15, column (L' & 3) + 4 k = (p >> 4) + 4 k of the second exchange, every entry of
    the 16 x 64 image once, inside the image the callers reserve (1088 entries) at a row stride of 65."""
    seen = set()
    for p in range(64):
        lv = virtual_lane(p)
        assert lv & 3 == p >> 4 and lv >> 2 == p & 15
        for k in range(16):
            y = (lv >> 2) * 64 + (lv & 3) + 4 * k             # the Stockham position pass 1 writes
            row, col = y >> 6, y & 63
            assert (row, col) == (p & 15, (p >> 4) + 4 * k)
            assert row * 65 + col == (p & 15) * 65 + (p >> 4) + 4 * k < 1088
            seen.add((row, col))
    assert len(seen) == 1024
    # the reader: physical lane q takes column q of every row
    assert max(q + 65 * r for q in range(64) for r in range(16)) < 1088


def test_second_exchange_store_groups_hit_every_bank_once():
    """An 8-byte LDS store is served in groups of 16 consecutive lanes over 32 four-byte banks.  The sixteen lanes of a group
    write sixteen rows of one column: at a row stride of 65 entries they cover all 32 banks; Pad<16>'s 68 would put them
    four deep."""
    def depth(stride):
        worst = 0
        for g in range(4):
            banks = {}
            for p in range(16 * g, 16 * g + 16):
                a = (p & 15) * stride + (p >> 4)              # entry address (8 bytes), k = 0
                for d in (2 * a, 2 * a + 1):
                    banks[d % 32] = banks.get(d % 32, 0) + 1
            worst = max(worst, max(banks.values()))
        return worst
    assert depth(65) == 1
    assert depth(68) == 4
