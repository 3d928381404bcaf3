"""The large-offset shape of the packed binned kernel, on the host.

Five bins of n = 4 << 24 rows of 16 words, 20 GiB: bin b's block starts at
flat row b * n, so bin 1 starts at byte 2^32, bin 2 at element 2^31 and bin 4
at element 2^32, the offset `bin * n * ROW` of the kernel's row base.  S is
chosen in the flat space of all 5 * n rows with the packed partner (rows r
and r ^ 4 are one lane of the two leaves of a pair) and cut into one
PackedSparseTable per bin, each with its own random rows, so a key that reads
another bin's block gives a different share.  test_packed_binned_cpu.py
checks by arithmetic where S lies; test_gpu_packed_binned.py runs it.
"""

import packed_oracle as po
import sparse_oracle as so

LARGE_D, LARGE_BINS, LARGE_WORDS = 24, 5, 16
LARGE_N = 4 << LARGE_D
LARGE_CROSSED = ["byte 2^31", "byte 2^32", "elem 2^31", "elem 2^32"]


def large_flat_rows(seed=0):
    return so.choose_rows(LARGE_BINS * LARGE_N, LARGE_WORDS, LARGE_N, seed,
                          po.other_leaf)


def large_bin_tables(flat=None):
    """One PackedSparseTable per bin; table b's prow are rows of ITS block
    (flat row b * n + prow)."""
    flat = large_flat_rows() if flat is None else flat
    n = LARGE_N
    return [po.PackedSparseTable(
        LARGE_D, 16, LARGE_WORDS, seed=70 + b,
        flat_rows=[r - b * n for r in flat if b * n <= r < (b + 1) * n])
        for b in range(LARGE_BINS)]
