"""Sparse oracle for tables and share matrices too large for a dense one.

The dense oracles (_core.eval_fused_cpu, _core.expand) need the whole table
or the whole share vector on the host.  Here the device table is zero except
for a small set S of rows, so the expected fused share of one key is

    sum over r in S of eval_point_low(key, r) * row_r   (mod 2^32)

which costs O(depth) per row of S whatever the table size.  S is built from
the rows that sit below, across and above every 32-bit offset boundary the
table crosses, so a kernel address that wraps there reads a zero row (or the
wrong written row) and the share differs.

Everything here is host arithmetic on Python ints and numpy: the row
permutation is restated from the layout contract

    row(idx) = j << (zlog + 1) | t << 1 | b
      t = the low zlog bits of idx, bit-reversed       (frontier position)
      j = the next depth - zlog - 1 bits, bit-reversed (DFS step)
      b = the top bit of idx                           (leaf of the pair)

and never calls the C++ leaf_perm; test_sparse_oracle.py compares the two.
"""

import numpy as np

from gpudpf import _core

# Offsets at which a 32-bit index wraps: (name, offset in u32 elements).
# A byte offset B is element offset B / 4.
BOUNDARIES = (
    ("byte 2^31", 1 << 29),
    ("byte 2^32", 1 << 30),
    ("elem 2^31", 1 << 31),
    ("elem 2^32", 1 << 32),
)
BOUNDARY = dict(BOUNDARIES)

EDGE_WORDS = np.array([0x80000000, 0xFFFFFFFF, 0, 1, 0x7FFFFFFF],
                      dtype=np.uint32)
N_RANDOM = 64


# ---------------------------------------------------------------------------
# The row permutation, stated in Python
# ---------------------------------------------------------------------------
def zlog_of(depth):
    """Z = 256 threads per unit, fewer for domains below 512."""
    return min(8, depth - 1)


def bitrev(v, bits):
    r = 0
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def leaf_perm(idx, depth, zlog):
    """Natural index -> permuted table row (Python ints)."""
    mid_bits = depth - zlog - 1
    t = bitrev(idx & ((1 << zlog) - 1), zlog)
    j = bitrev((idx >> zlog) & ((1 << mid_bits) - 1), mid_bits)
    b = idx >> (depth - 1)
    return (j << (zlog + 1)) | (t << 1) | b


def leaf_perm_inv(row, depth, zlog):
    """Permuted table row -> natural index (Python ints)."""
    mid_bits = depth - zlog - 1
    b = row & 1
    t = (row >> 1) & ((1 << zlog) - 1)
    j = row >> (zlog + 1)
    return (bitrev(t, zlog) | (bitrev(j, mid_bits) << zlog)
            | (b << (depth - 1)))


# ---------------------------------------------------------------------------
# Choosing S in a flat space of rows
# ---------------------------------------------------------------------------
def _adjacent(r):
    """Rows 2m and 2m + 1 are leaves b = 0, 1 of the same (j, t)."""
    return r ^ 1


def crossed(total_rows, row_words):
    """The boundaries a flat array of total_rows rows of row_words u32
    crosses STRICTLY: it holds an element at an offset >= the boundary."""
    last = total_rows * row_words - 1
    return [name for name, off in BOUNDARIES if last >= off]


def boundary_rows(off, row_words):
    """(last row wholly below, rows containing, first row wholly above)
    element offset `off`.  A row contains the boundary when it has elements
    on both sides; a row that starts exactly at it is wholly above."""
    q, rem = divmod(off, row_words)
    if rem == 0:
        return q - 1, [], q
    return q - 1, [q], q + 1


def choose_rows(total_rows, row_words, block_rows, seed, partner=_adjacent):
    """Sorted flat row indices of S for an array of total_rows rows of
    row_words u32, made of blocks of block_rows rows (one table, the bins of
    a binned table, or the keys of a share matrix):

      * the first and last row of every block;
      * for every boundary crossed, the last row wholly below it, every row
        containing it and the first row wholly above it;
      * the partner of each of those and the two rows beyond on each side
        with theirs, so that both rows of a leaf pair lie wholly on each
        side of each boundary;
      * N_RANDOM seeded random rows per block.
    """
    assert total_rows % block_rows == 0
    rows = set()
    for blk in range(total_rows // block_rows):
        rows.add(blk * block_rows)
        rows.add((blk + 1) * block_rows - 1)
    for name in crossed(total_rows, row_words):
        below, holds, above = boundary_rows(BOUNDARY[name], row_words)
        near = [below - 2, below - 1, below] + holds + \
            [above, above + 1, above + 2]
        for r in near:
            rows.add(r)
            rows.add(partner(r))
    rng = np.random.default_rng(seed)
    for blk in range(total_rows // block_rows):
        for r in rng.integers(0, block_rows, N_RANDOM):
            rows.add(blk * block_rows + int(r))
    return sorted(r for r in rows if 0 <= r < total_rows)


def straddle_report(rows, total_rows, row_words, partner=_adjacent):
    """For each boundary crossed: what S holds around it.  Pure arithmetic;
    the tests assert on it."""
    have = set(rows)
    rep = {}
    for name in crossed(total_rows, row_words):
        off = BOUNDARY[name]
        below = {r for r in rows if (r + 1) * row_words <= off}
        above = {r for r in rows if r * row_words >= off}
        holds = [r for r in rows
                 if r * row_words < off < (r + 1) * row_words]
        want_below, want_holds, want_above = boundary_rows(off, row_words)

        def pair_in(side):
            return any(partner(r) != r and partner(r) in side for r in side)

        rep[name] = {
            "last_below": want_below in have and max(below) == want_below,
            "first_above": want_above in have and min(above) == want_above,
            "holds": holds == want_holds,
            "pair_below": pair_in(below),
            "pair_above": pair_in(above),
        }
    return rep


# ---------------------------------------------------------------------------
# Rows, keys and expected shares
# ---------------------------------------------------------------------------
def random_rows(m, e, seed):
    """[m, e] int32 rows from a seeded generator; about one word in eight is
    an edge value, and 0x80000000 and 0xFFFFFFFF are certain to occur."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << 32, (m, e), dtype=np.uint64).astype(np.uint32)
    edge = rng.choice(EDGE_WORDS, (m, e))
    rows = np.where(rng.integers(0, 8, (m, e)) == 0, edge, rows)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    rows.reshape(-1)[0] = 0x80000000
    rows.reshape(-1)[-1] = 0xFFFFFFFF
    return rows.view(np.int32)


def gen_keys(alphas, n, prf, seed):
    """One key pair per alpha from a seeded generator: ([k1...], [k2...])
    as int32[524] numpy arrays."""
    rng = np.random.default_rng(seed)
    k1s, k2s = [], []
    for a in alphas:
        s = bytes(rng.integers(0, 256, 128, dtype=np.uint8))
        k1, k2 = _core.gen(int(a), n, s, prf)
        k1s.append(k1)
        k2s.append(k2)
    return k1s, k2s


def point_shares(key, indices, prf):
    """Low 32 bits of the key's share at each natural index, as uint64."""
    return np.array([_core.eval_point_low(key, int(i), prf) for i in indices],
                    dtype=np.uint64)


def sparse_share(key, indices, rows, prf):
    """Expected fused share int32[e] of `key` against a table that is zero
    except rows[i] at natural index indices[i]: wrapping uint64 arithmetic,
    truncated to 32 bits."""
    v = point_shares(key, indices, prf)
    r = rows.view(np.uint32).astype(np.uint64)
    acc = (v[:, None] * r).sum(axis=0, dtype=np.uint64)
    return acc.astype(np.uint32).view(np.int32)


def reconstruct(a, b):
    """(a - b) mod 2^32 of two int32 share arrays."""
    return (a.astype(np.int64) - b.astype(np.int64)).astype(np.uint32) \
        .view(np.int32)


class SparseTable:
    """S for one table of n = 2^depth rows of e words (row stride
    row_words, the padded width), optionally one block of a binned table
    that starts at flat row `base`.

    nat[i] is the natural index of permuted row prow[i] (flat row base +
    prow[i]); rows[i] the int32[e] row written there."""

    def __init__(self, depth, e, row_words, seed, flat_rows=None, base=0):
        self.depth, self.e, self.row_words = depth, e, row_words
        self.n = 1 << depth
        self.zlog = zlog_of(depth)
        if flat_rows is None:
            flat_rows = choose_rows(self.n, row_words, self.n, seed)
        self.prow = [r - base for r in flat_rows
                     if base <= r < base + self.n]
        self.nat = np.array([leaf_perm_inv(r, depth, self.zlog)
                             for r in self.prow], dtype=np.int64)
        self.rows = random_rows(len(self.prow), e, seed + 1)

    def share(self, key, prf):
        return sparse_share(key, self.nat, self.rows, prf)

    def row_of(self, alpha):
        (i,) = np.nonzero(self.nat == alpha)[0]
        return self.rows[i]

    def dense(self):
        t = np.zeros((self.n, self.e), dtype=np.int32)
        t[self.nat] = self.rows
        return t

    def alphas(self, count):
        """`count` distinct members of S to serve as keys' secret indices:
        the natural index of the highest row first (above every boundary),
        then of row 0, then spread evenly over S."""
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


# ---------------------------------------------------------------------------
# The shapes the GPU tests use, for the boundary-arithmetic tests
# ---------------------------------------------------------------------------
def half_partner(block_rows):
    """Partner in a natural-order share row: the breadth-first kernel writes
    leaves p and p + n/2 from one parent."""
    return lambda r: r ^ (block_rows >> 1)


ALL_FOUR = ["byte 2^31", "byte 2^32", "elem 2^31", "elem 2^32"]

# name -> (total_rows, row_words, block_rows, boundaries claimed, partner)
GPU_SHAPES = {
    # fused tables: rows of the padded width
    "fused_w4_n24": (1 << 24, 64, 1 << 24, ["byte 2^31"], _adjacent),
    "fused_w3_n27": (1 << 27, 48, 1 << 27, ALL_FOUR, _adjacent),
    "fused_d28": (1 << 28, 16, 1 << 28,
                  ["byte 2^31", "byte 2^32", "elem 2^31"], _adjacent),
    "binned_5x_n26": (5 << 26, 16, 1 << 26, ALL_FOUR, _adjacent),
    # share matrices: one u32 per position, one block per key
    "expand_b5_n30": (5 << 30, 1, 1 << 30, ALL_FOUR, _adjacent),
    "bfs_b3_n28": (3 << 28, 1, 1 << 28, ["byte 2^31"],
                   half_partner(1 << 28)),
    # GEMM operand b [K, N]
    "gemm_b": ((1 << 26) + 65, 68, (1 << 26) + 65, ALL_FOUR, _adjacent),
    "two_stage_n26_e80": (1 << 26, 80, 1 << 26, ALL_FOUR, _adjacent),
}


def shape_rows(name, seed=0):
    total, words, block, _claims, partner = GPU_SHAPES[name]
    return choose_rows(total, words, block, seed, partner)
