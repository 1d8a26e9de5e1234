"""The group footprint's mask as two v_bitop3 a word with a zero row (tracer.hip group_foot_mask,
kFootBitop) against the form it replaces, in numpy.

The parent combined the four table rows word by word as `a & b & c & e`, selected 0 for a ray that
never reaches the y extent (`none`) and or-ed `always` in. The kernel now reads the tables' zero
row in place of row a for such a ray (one select on the index) and forms each word by
bitop3(bitop3(a, b, c, kBitopAnd3), e, always, kBitopAndOr). Both must give the same bits for every
input. The two truth-table bytes are read from vcrt_kernel_abi.h and held against a 256-entry
evaluation of v_bitop3's rule: bit 4x + 2y + z of the byte is the result for operand bits x, y, z.
The zero row's place in the LDS image (group_foot_zero_pad) is checked for every group count the
tables admit.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc", "vcrt_kernel_abi.h")


def table_byte(name):
    with open(ABI) as f:
        m = re.search(r"constexpr uint32_t %s = (0x[0-9a-fA-F]+);" % name, f.read())
    assert m, name
    return int(m.group(1), 16)


def bitop3(x, y, z, tt):
    """v_bitop3_b32 on uint32 arrays: result bit = bit (4x + 2y + z) of the table byte."""
    x, y, z = (np.asarray(v, np.uint32) for v in (x, y, z))
    out = np.zeros(np.broadcast(x, y, z).shape, np.uint32)
    for i in range(8):
        if (tt >> i) & 1:
            out |= ((x if i & 4 else ~x) & (y if i & 2 else ~y) & (z if i & 1 else ~z))
    return out


def test_truth_table_bytes():
    and3, andor = table_byte("kBitopAnd3"), table_byte("kBitopAndOr")
    # the byte from the function, entry by entry
    want_and3 = sum((x & y & z) << (4 * x + 2 * y + z)
                    for x in (0, 1) for y in (0, 1) for z in (0, 1))
    want_andor = sum(((x & y) | z) << (4 * x + 2 * y + z)
                     for x in (0, 1) for y in (0, 1) for z in (0, 1))
    assert (and3, andor) == (want_and3, want_andor) == (0x80, 0xEA)
    # all 256 tables on all operand bits: the model is the rule, and only these two bytes are
    # the two functions
    x = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.uint32)
    y = np.array([0, 0, 1, 1, 0, 0, 1, 1], np.uint32)
    z = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.uint32)
    for tt in range(256):
        got = bitop3(x, y, z, tt) & 1
        assert [int(v) for v in got] == [(tt >> i) & 1 for i in range(8)], tt
        assert np.array_equal(got, x & y & z) == (tt == and3), tt
        assert np.array_equal(got, (x & y) | z) == (tt == andor), tt


def test_two_bitops_and_the_zero_row_equal_the_select_form():
    rng = np.random.default_rng(14)
    n_rows, n = 94, 1 << 20
    # a table of 128-bit rows: random, sparse, dense, all-ones and all-zero rows, then the zero row
    tab = rng.integers(0, 1 << 32, (n_rows, 4), dtype=np.uint64).astype(np.uint32)
    tab[10:30] &= rng.integers(0, 1 << 32, (20, 4), dtype=np.uint64).astype(np.uint32)
    tab[30:50] |= rng.integers(0, 1 << 32, (20, 4), dtype=np.uint64).astype(np.uint32)
    tab[50:60] = 0xFFFFFFFF
    tab[60:66] = 0
    zero_row = n_rows
    tab = np.vstack([tab, np.zeros((1, 4), np.uint32)])
    ia, ib, ic, ie = (rng.integers(0, n_rows, n) for _ in range(4))
    # rows of all ones in every place for a share of the rays: the and keeps every bit
    ones = rng.random(n) < 0.05
    for idx in (ia, ib, ic, ie):
        idx[ones] = 50
    none = rng.random(n) < 0.3
    always = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    always[rng.random(n) < 0.4] = 0  # a scene without such groups
    always[rng.random(n) < 0.05] = 0xFFFFFFFF
    assert (none & (always != 0).any(axis=1)).sum() > 1000 and (none & ones).sum() > 1000
    a, b, c, e = tab[ia], tab[ib], tab[ic], tab[ie]
    want = np.where(none[:, None], np.uint32(0), a & b & c & e) | always
    az = tab[np.where(none, zero_row, ia)]
    got = bitop3(bitop3(az, b, c, table_byte("kBitopAnd3")), e, always, table_byte("kBitopAndOr"))
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(got[none], always[none])


def test_zero_row_lies_ahead_of_the_group_records():
    """vcrt_kernel_abi.h restated: the four tables of group_foot_cells 16-B cells and the zero row
    fit in the float4s of the boxes and node tables they replace plus group_foot_zero_pad."""
    with open(ABI) as f:
        text = f.read()
    assert "return bytes - 64u * group_foot_cells(ncgroups) >= 16u ? 0u : 1u;" in text
    for ncgroups in range(8, 129, 8):
        foot = 4 * 84 * (4 if ncgroups > 128 else 2)
        bytes_ = ncgroups // 8 * 336 + foot
        cells = bytes_ // 64
        pad = 0 if bytes_ - 64 * cells >= 16 else 1
        assert 64 * cells + 16 <= bytes_ + 16 * pad, ncgroups
        assert pad == (1 if ncgroups // 8 % 4 == 2 else 0), ncgroups
    assert (128 // 8 * 336 + 672) - 64 * 94 == 32  # the final scene: no pad, the image's size kept
