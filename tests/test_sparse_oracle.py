"""The sparse oracle (tests/sparse_oracle.py) against the C++ core, and the
arithmetic that the large-offset GPU tests (test_gpu_large_offsets.py) rest
on.  No GPU needed."""

import numpy as np
import pytest

import sparse_oracle as so
from gpudpf import DPF, _core

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}


@pytest.mark.parametrize("depth", range(7, 15))
def test_python_perm_equals_core_everywhere(depth):
    n = 1 << depth
    zlog = so.zlog_of(depth)
    assert zlog == _core.zlog_for_depth(depth)
    mine = np.array([so.leaf_perm(i, depth, zlog) for i in range(n)],
                    dtype=np.int64)
    assert np.array_equal(mine, _core.leaf_perm_table(n, zlog))
    assert np.array_equal(
        mine, _core.leaf_perm_rows(np.arange(n, dtype=np.int64), n, zlog))
    # a permutation, and the stated inverse inverts it
    assert np.array_equal(np.sort(mine), np.arange(n))
    back = [so.leaf_perm_inv(int(r), depth, zlog) for r in mine]
    assert back == list(range(n))


@pytest.mark.parametrize("depth", range(24, 31))
def test_python_perm_equals_core_sampled(depth):
    n = 1 << depth
    zlog = so.zlog_of(depth)
    assert zlog == _core.zlog_for_depth(depth)
    rng = np.random.default_rng(depth)
    idx = np.concatenate([
        rng.integers(0, n, 2000),
        [0, 1, n - 1, n - 2, n >> 1, (n >> 1) - 1, 255, 256, 257],
        1 << np.arange(depth)])
    idx = idx.astype(np.int64)
    mine = np.array([so.leaf_perm(int(i), depth, zlog) for i in idx],
                    dtype=np.int64)
    assert np.array_equal(mine, _core.leaf_perm_rows(idx, n, zlog))
    assert [so.leaf_perm_inv(int(r), depth, zlog) for r in mine] \
        == [int(i) for i in idx]


@pytest.mark.parametrize("depth", [10, 11, 12])
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_sparse_oracle_equals_dense_core(prf, depth):
    n = 1 << depth
    for e in (16, 48):
        st = so.SparseTable(depth, e, e, seed=depth * 10 + prf)
        assert len(set(st.nat.tolist())) == len(st.nat) >= so.N_RANDOM // 2
        dense = st.dense()
        words = st.rows.view(np.uint32)
        assert (words == 0x80000000).any() and (words == 0xFFFFFFFF).any()
        alphas = st.alphas(3)
        assert set(alphas) <= set(st.nat.tolist())
        k1s, k2s = so.gen_keys(alphas, n, prf, seed=depth + 100 * prf)
        for a, k1, k2 in zip(alphas, k1s, k2s):
            s1, s2 = st.share(k1, prf), st.share(k2, prf)
            assert np.array_equal(s1, _core.eval_fused_cpu(k1, dense, prf))
            assert np.array_equal(s2, _core.eval_fused_cpu(k2, dense, prf))
            assert np.array_equal(so.reconstruct(s1, s2), dense[a])
            assert np.array_equal(st.row_of(a), dense[a])


def test_point_shares_equal_expand():
    depth, prf = 10, DPF.PRF_CHACHA20
    (k1,), _ = so.gen_keys([77], 1 << depth, prf, seed=5)
    idx = np.arange(1 << depth)
    want = _core.expand(k1, prf).view(np.uint32).astype(np.uint64)
    assert np.array_equal(so.point_shares(k1, idx, prf), want)


def test_boundary_rows_cases():
    # aligned: no row holds the boundary, the row starting there is above
    assert so.boundary_rows(1 << 29, 16) == ((1 << 25) - 1, [], 1 << 25)
    # 48-word rows straddle every power of two
    below, holds, above = so.boundary_rows(1 << 32, 48)
    assert holds == [below + 1] and above == below + 2
    assert (below + 1) * 48 < (1 << 32) < (below + 2) * 48
    # exactly 2^32 elements reaches the boundary and crosses nothing
    assert "elem 2^32" not in so.crossed(1 << 28, 16)
    assert "elem 2^32" in so.crossed((1 << 28) + 1, 16)
    assert so.crossed(1 << 24, 64) == ["byte 2^31"]


@pytest.mark.parametrize("name", sorted(so.GPU_SHAPES))
def test_gpu_shape_straddles_what_it_claims(name):
    total, words, block, claims, partner = so.GPU_SHAPES[name]
    # the table exceeds each claimed boundary strictly, and claims them all
    assert so.crossed(total, words) == claims
    for c in claims:
        assert total * words - 1 >= so.BOUNDARY[c]
    rows = so.shape_rows(name)
    assert rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < total
    assert rows[0] == 0 and rows[-1] == total - 1
    for blk in range(total // block):
        assert blk * block in rows and (blk + 1) * block - 1 in rows
        inside = [r for r in rows if blk * block <= r < (blk + 1) * block]
        assert len(inside) >= so.N_RANDOM // 2
    rep = so.straddle_report(rows, total, words, partner)
    assert sorted(rep) == sorted(claims)
    for c, facts in rep.items():
        assert all(facts.values()), (name, c, facts)
    # at least one row lies above the highest boundary
    top = max(so.BOUNDARY[c] for c in claims)
    assert rows[-1] * words >= top
    assert len(rows) < 1000


def test_gpu_table_shapes_give_alphas_above_the_top_boundary():
    for name, depth, e in (("fused_w4_n24", 24, 64), ("fused_w3_n27", 27, 48),
                           ("fused_d28", 28, 16),
                           ("two_stage_n26_e80", 26, 80)):
        total, words, _block, claims, _p = so.GPU_SHAPES[name]
        assert total == 1 << depth and words == e
        st = so.SparseTable(depth, e, words, seed=1,
                            flat_rows=so.shape_rows(name))
        alphas = st.alphas(3)
        assert len(set(alphas)) == 3 and set(alphas) <= set(st.nat.tolist())
        top = max(so.BOUNDARY[c] for c in claims)
        row = so.leaf_perm(alphas[0], depth, st.zlog)
        assert row * words >= top
        # S keeps both leaves b = 0, 1 of one (j, t): a pair of adjacent rows
        assert any(r + 1 in st.prow for r in st.prow if r % 2 == 0)
