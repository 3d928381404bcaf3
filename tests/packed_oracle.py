"""Host-side statements of the packed layout for the packed-key tests.

The row of natural index idx in a packed table of n = 4 * 2^D rows (D the
tree depth, zlog = zlog_of(D)):

    node = idx & (2^D - 1)      lane = idx >> D
    row  = j << (zlog + 3) | t << 3 | b << 2 | lane
      t = the low zlog bits of node, bit-reversed
      j = the next D - zlog - 1 bits of node, bit-reversed
      b = the top bit of node

restated here on Python ints; it never calls the C++ packed_perm, and
test_packed_cpu.py compares the two.  PackedSparseTable is sparse_oracle's
SparseTable for that layout: a device table that is zero except a set S of
rows around every 32-bit offset boundary, with the expected share summed
from eval_point_low.
"""

import numpy as np

import sparse_oracle as so
from sparse_oracle import bitrev
from gpudpf import _core


def packed_perm(idx, D, zlog):
    node, lane = idx & ((1 << D) - 1), idx >> D
    mid_bits = D - zlog - 1
    t = bitrev(node & ((1 << zlog) - 1), zlog)
    j = bitrev((node >> zlog) & ((1 << mid_bits) - 1), mid_bits)
    b = node >> (D - 1)
    return (j << (zlog + 3)) | (t << 3) | (b << 2) | lane


def packed_perm_inv(row, D, zlog):
    mid_bits = D - zlog - 1
    lane, b = row & 3, (row >> 2) & 1
    t = (row >> 3) & ((1 << zlog) - 1)
    j = row >> (zlog + 3)
    node = bitrev(t, zlog) | (bitrev(j, mid_bits) << zlog) | (b << (D - 1))
    return node | (lane << D)


def other_leaf(r):
    """Rows r and r ^ 4 are the same lane of the two leaves of one pair."""
    return r ^ 4


def gen_keys(alphas, n, prf, seed):
    """One packed key pair per alpha from a seeded generator."""
    rng = np.random.default_rng(seed)
    k1s, k2s = [], []
    for a in alphas:
        s = bytes(rng.integers(0, 256, 128, dtype=np.uint8))
        k1, k2 = _core.gen(int(a), n, s, prf, packed=True)
        k1s.append(k1)
        k2s.append(k2)
    return k1s, k2s


def lane_alphas(n, count, seed):
    """`count` >= 6 distinct indices: 0, n - 1, one in each lane, the rest
    seeded random."""
    rng = np.random.default_rng(seed)
    q = n // 4
    out = [0, n - 1] + [k * q + int(rng.integers(1, q - 1)) for k in range(4)]
    while len(out) < count:
        a = int(rng.integers(0, n))
        if a not in out:
            out.append(a)
    assert len(set(out)) == len(out) >= 6
    assert {a // q for a in out} == {0, 1, 2, 3}
    return out[:count]


# The large-offset shape of test_gpu_packed.py: 2^27 rows of 16 words, 8 GiB.
# It crosses bytes 2^31 and 2^32 and ends exactly at element 2^31.
LARGE_D, LARGE_WORDS = 25, 16
LARGE_CROSSED = ["byte 2^31", "byte 2^32"]


def large_rows(seed=0):
    """choose_rows, plus the other leaf of the last row (the table's end is
    element 2^31)."""
    n = 4 << LARGE_D
    rows = set(so.choose_rows(n, LARGE_WORDS, n, seed, other_leaf))
    rows.add(other_leaf(n - 1))
    return sorted(rows)


class PackedSparseTable:
    """S for one packed table of n = 4 << D rows of e words: nat[i] is the
    natural index of table row prow[i], rows[i] the int32[e] row there."""

    def __init__(self, D, e, row_words, seed, flat_rows=None):
        self.D, self.e, self.row_words = D, e, row_words
        self.n = 4 << D
        self.zlog = so.zlog_of(D)
        if flat_rows is None:
            flat_rows = so.choose_rows(self.n, row_words, self.n, seed,
                                       other_leaf)
        self.prow = list(flat_rows)
        self.nat = np.array([packed_perm_inv(r, D, self.zlog)
                             for r in self.prow], dtype=np.int64)
        self.rows = so.random_rows(len(self.prow), e, seed + 1)

    def share(self, key, prf):
        return so.sparse_share(key, self.nat, self.rows, prf)

    def row_of(self, alpha):
        (i,) = np.nonzero(self.nat == alpha)[0]
        return self.rows[i]

    def alphas(self, count):
        """The natural index of the highest row (above every boundary),
        of row 0, then spread evenly over S."""
        order = [len(self.nat) - 1, 0]
        step = max(1, len(self.nat) // max(1, count))
        order += list(range(step // 2, len(self.nat), step))
        seen, out = set(), []
        for i in order:
            a = int(self.nat[i])
            if a not in seen:
                seen.add(a)
                out.append(a)
        return out[:count]
