"""The eval kernels and the stream GEMM past depth 20 and past 32-bit offsets.

test_gpu_eval_lattice.py is exact but dense: it ends at depth 20 (DS 12, five
global sibling-stack levels) and inside the first 64 MiB of a table.  Here
the tables are zero on the device except a sparse set S of rows, and one
server's share is compared exactly with the sparse oracle
(tests/sparse_oracle.py), so a check costs O(depth) per row of S whatever
the table size.  test_sparse_oracle.py proves on the CPU that each S below
holds rows below, across and above every boundary its shape crosses.

  depth 21, 22, 24   all four PRFs, DS 13..16 (6..9 global levels), slog 8
                     (batch 3) and slog 2 (batch 257); caller-owned scratch
                     and the expand kernel at depth 24
  depth 28           AES and ChaCha, DS 20, a 16 GiB table: the first real
                     domain above DPF.PERM_MATERIALIZE_MAX
  2^31 / 2^32        fused W=4 and W=3 rows, the binned block offset, the
                     expand and breadth-first share matrices, the stream
                     GEMM directly and through the two-stage dispatch

Peak device memory is stated per test (PEAK GiB, by arithmetic from the
shapes; none exceeds 32) and a test skips only when the device reports less
than that plus 4 GiB free.  Every comparison is exact.
"""

import functools
import gc

import numpy as np
import pytest
import torch

import sparse_oracle as so
from gpudpf import DPF, _core, ops

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

pytestmark = pytest.mark.gpu

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
N_KEYS = 5
GIB = 1 << 30


def _need(peak_gib):
    """Skip only when the device cannot hold the test's peak plus 4 GiB."""
    _release()
    free, _total = torch.cuda.mem_get_info()
    if free < (peak_gib + 4) * GIB:
        pytest.skip("needs %d GiB of free device memory (peak %d GiB + 4), "
                    "%.1f GiB free" % (peak_gib + 4, peak_gib, free / GIB))


def _release():
    gc.collect()
    torch.cuda.empty_cache()


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _batch_of(keys, batch):
    return torch.from_numpy(np.stack([keys[i % len(keys)]
                                      for i in range(batch)]))


@functools.lru_cache(maxsize=None)
def _sparse(name_or_depth, e, words):
    """S and its rows for one table shape; built once, never modified."""
    if isinstance(name_or_depth, str):
        total = so.GPU_SHAPES[name_or_depth][0]
        depth = total.bit_length() - 1
        assert total == 1 << depth
        return so.SparseTable(depth, e, words, seed=depth * 100 + e,
                              flat_rows=so.shape_rows(name_or_depth))
    return so.SparseTable(name_or_depth, e, words,
                          seed=name_or_depth * 100 + e)


@functools.lru_cache(maxsize=None)
def _case(prf, st):
    """N_KEYS key pairs with alphas in S (the first above every boundary)
    and both servers' oracle shares."""
    alphas = st.alphas(N_KEYS)
    assert len(alphas) == N_KEYS
    k1s, k2s = so.gen_keys(alphas, st.n, prf, seed=prf * 1000 + st.depth)
    want1 = np.stack([st.share(k, prf) for k in k1s])
    want2 = np.stack([st.share(k, prf) for k in k2s])
    secret = np.stack([st.row_of(a) for a in alphas])
    assert np.array_equal(so.reconstruct(want1, want2), secret)  # the oracle
    return alphas, k1s, k2s, want1, want2, secret


def _engine(prf, st, fused_words=16):
    """Engine with the zeroed device table and S written through
    table_write; table_read must give S back."""
    dpf = DPF(prf=prf, fused_words=fused_words)
    dpf.eval_init_empty(st.n, st.e)
    assert dpf._entry_padded == st.row_words and dpf._zlog == st.zlog
    nat = torch.from_numpy(st.nat)
    dpf.table_write(nat, torch.from_numpy(st.rows))
    assert np.array_equal(dpf.table_read(nat).cpu().numpy(), st.rows)
    # the rows landed where the Python permutation says, nowhere else
    prow = torch.tensor(st.prow, dtype=torch.int64, device=_dev())
    assert np.array_equal(dpf._table_gpu[prow, :st.e].cpu().numpy(), st.rows)
    return dpf


def _check_fused(dpf, prf, st, batch, slog):
    """One server's GPU shares == the oracle's, and a - b == table[alpha]
    from a GPU share and an oracle share."""
    _alphas, k1s, _k2s, want1, want2, secret = _case(prf, st)
    depth, zlog = st.depth, st.zlog
    assert _hip.eval_slog(batch, depth, zlog) == slog, (depth, batch)
    units = batch << slog
    assert _hip.eval_scratch_bytes(batch, depth, zlog) \
        == units * (depth - zlog - 7) * 256 * 16
    idx = np.arange(batch) % N_KEYS
    got = dpf.eval_gpu(_batch_of(k1s, batch)).numpy()
    assert np.array_equal(got, want1[idx]), (depth, batch)
    assert np.array_equal(so.reconstruct(got, want2[idx]), secret[idx])
    return got


# ---------------------------------------------------------------------------
# Depth 21..28: the DS axis past the lattice's 12
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [21, 22, 24])
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_deep_fused_matches_sparse_oracle(prf, depth, monkeypatch):
    """PEAK 2 GiB: the 1 GiB table at depth 24 and its row permutation."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _need(2)
    st = _sparse(depth, 16, 16)
    assert so.crossed(st.n, 16) == []  # deep, not large
    dpf = _engine(prf, st)
    assert dpf._perm_gpu is not None
    _check_fused(dpf, prf, st, batch=3, slog=8)
    _check_fused(dpf, prf, st, batch=257, slog=2)
    dpf.eval_free()
    _release()


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_depth28_fused_matches_sparse_oracle(prf, monkeypatch):
    """PEAK 16 GiB: n = 2^28 rows of 16 words, 2^32 elements, which crosses
    bytes 2^31 and 2^32 and element 2^31 and only reaches element 2^32.  The
    domain is above PERM_MATERIALIZE_MAX, so table_write, table_read and
    _rows take the chunk-wise permutation for real."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _need(16)
    st = _sparse("fused_d28", 16, 16)
    assert st.n > DPF.PERM_MATERIALIZE_MAX
    dpf = _engine(prf, st)
    assert dpf._perm_gpu is None
    _check_fused(dpf, prf, st, batch=3, slog=8)
    dpf.eval_free()
    _release()


def test_gpu_depth24_caller_owned_scratch():
    """PEAK 2 GiB.  The same launch with the sibling stack in a buffer of
    exactly _scratch_bytes that the caller owns."""
    _need(2)
    prf = DPF.PRF_DUMMY
    st = _sparse(24, 16, 16)
    dpf = _engine(prf, st)
    batch = 3
    shared = _check_fused(dpf, prf, st, batch=batch, slog=8)
    _alphas, k1s, _k2s, want1, _w2, _s = _case(prf, st)
    keys_gpu = _batch_of(k1s, batch).to(_dev())
    need = dpf._scratch_bytes(batch)
    assert need == (batch << 8) * 9 * 256 * 16
    scratch = torch.empty(need, dtype=torch.uint8, device=_dev())
    out = torch.zeros((batch, 16), dtype=torch.int32, device=_dev())
    dpf._launch_fused(keys_gpu, out, scratch=scratch)
    own = out.cpu().numpy()
    assert np.array_equal(own, shared)
    assert np.array_equal(own, want1[:batch])
    del scratch, out
    dpf.eval_free()
    _release()


@pytest.mark.parametrize("batch,slog", [(3, 8), (65, 4)])
def test_gpu_depth24_expand_matches_point_shares(batch, slog):
    """PEAK 6 GiB: 65 share rows of 64 MiB beside the table.  The share
    matrix stays on the device; only the positions of S come back."""
    _need(6)
    prf = DPF.PRF_DUMMY
    st = _sparse(24, 16, 16)
    dpf = _engine(prf, st)
    _alphas, k1s, _k2s, _w1, _w2, _s = _case(prf, st)
    assert _hip.eval_slog(batch, 24, 8) == slog
    keys_gpu = _batch_of(k1s, batch).to(_dev())
    shares = torch.empty((batch, st.n), dtype=torch.int32, device=_dev())
    dpf._launch_expand(keys_gpu, shares)
    pos = torch.tensor(st.prow, dtype=torch.int64, device=_dev())
    got = shares.index_select(1, pos).cpu().numpy().view(np.uint32)
    want = np.stack([so.point_shares(k, st.nat, prf) for k in k1s])
    assert np.array_equal(got.astype(np.uint64),
                          want[np.arange(batch) % N_KEYS])
    del shares
    dpf.eval_free()
    _release()


# ---------------------------------------------------------------------------
# Offsets past 2^31 and 2^32
# ---------------------------------------------------------------------------
def test_gpu_fused_w4_crosses_byte_2_31():
    """PEAK 5 GiB: n = 2^24 rows of 64 words = 4 GiB.  Crosses byte 2^31;
    byte 2^32 is reached, not crossed."""
    _need(5)
    prf = DPF.PRF_DUMMY
    st = _sparse("fused_w4_n24", 64, 64)
    dpf = _engine(prf, st, fused_words=64)
    assert dpf.fused_servable
    _check_fused(dpf, prf, st, batch=3, slog=8)
    dpf.eval_free()
    _release()


def test_gpu_fused_w3_crosses_every_boundary(monkeypatch):
    """PEAK 24 GiB: n = 2^27 rows of 48 words, 6.4e9 elements.  48-word rows
    straddle every power of two, so bytes 2^31 and 2^32 and elements 2^31
    and 2^32 each fall inside a row of S.  AES: its wide kernel has K <= 2
    instantiations of its own.  The row permutation is left on the host
    (seven seconds of a bit-reversal loop to build at this size); the depth
    24 tests above run with it on the device."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    monkeypatch.setattr(DPF, "PERM_MATERIALIZE_MAX", 1 << 24)
    _need(24)
    prf = DPF.PRF_AES128
    st = _sparse("fused_w3_n27", 48, 48)
    dpf = _engine(prf, st, fused_words=48)
    assert dpf.fused_servable
    assert _hip.eval_units_per_wg(prf, 3 << 8, 48) == 2
    _check_fused(dpf, prf, st, batch=3, slog=8)
    dpf.eval_free()
    _release()


def test_gpu_binned_block_offset_past_2_32_elements():
    """PEAK 20 GiB: 5 bins of n = 2^26 rows of 16 words.  Bin 4's block
    starts at element 2^32, bin 2's at element 2^31, bin 1's at byte 2^32.
    Every bin holds its own S, so a key that reads another bin's block (or a
    block offset that wrapped to bin 0) gives a different share."""
    _need(20)
    prf = DPF.PRF_DUMMY
    depth, bins = 26, [4, 0, 2, 4, 1]
    n, zlog = 1 << depth, 8
    flat = so.shape_rows("binned_5x_n26")
    sts = [so.SparseTable(depth, 16, 16, seed=50 + b, flat_rows=flat,
                          base=b * n) for b in range(5)]
    table = torch.zeros((5 * n, 16), dtype=torch.int32, device=_dev())
    for b, st in enumerate(sts):
        rows = torch.tensor([b * n + r for r in st.prow], dtype=torch.int64,
                            device=_dev())
        table[rows] = torch.from_numpy(st.rows).to(_dev())
        assert np.array_equal(table[rows].cpu().numpy(), st.rows)
    # key i selects a member of its own bin's S, the highest row first
    alphas = [sts[b].alphas(2)[i // 3] for i, b in enumerate(bins)]
    assert so.leaf_perm(alphas[0], depth, zlog) == n - 1  # last row, bin 4
    k1s, k2s = so.gen_keys(alphas, n, prf, seed=26)
    want1 = np.stack([sts[b].share(k, prf) for b, k in zip(bins, k1s)])
    want2 = np.stack([sts[b].share(k, prf) for b, k in zip(bins, k2s)])
    secret = np.stack([sts[b].row_of(a) for b, a in zip(bins, alphas)])
    assert np.array_equal(so.reconstruct(want1, want2), secret)
    # the shares tell the bins apart
    other = np.stack([sts[(b + 1) % 5].share(k, prf)
                      for b, k in zip(bins, k1s)])
    assert not (other == want1).all(axis=1).any()

    keys_gpu = torch.from_numpy(np.stack(k1s)).to(_dev())
    bins_gpu = torch.tensor(bins, dtype=torch.int32, device=_dev())
    out = torch.zeros((5, 16), dtype=torch.int32, device=_dev())
    assert _hip.eval_slog(5, depth, zlog) == 8
    _hip.eval_fused_binned(keys_gpu.data_ptr(), table.data_ptr(),
                           bins_gpu.data_ptr(), out.data_ptr(), 0, 5, n,
                           depth, zlog, 5, prf, _stream(), 0, 0, 16)
    got = out.cpu().numpy()
    assert np.array_equal(got, want1)
    assert np.array_equal(so.reconstruct(got, want2), secret)
    del table, out
    _release()


def test_gpu_expand_key_offset_past_2_32_elements():
    """PEAK 20 GiB: batch 5 at n = 2^30.  Keys 2..4 write at element
    offsets from 2^31 to past 2^32; S is chosen in the flat share matrix
    and holds positions of every key."""
    _need(20)
    prf = DPF.PRF_DUMMY
    depth, batch = 30, 5
    n, zlog = 1 << depth, 8
    flat = so.shape_rows("expand_b5_n30")
    assert {f >> depth for f in flat} == set(range(batch))
    nat = [so.leaf_perm_inv(f & (n - 1), depth, zlog) for f in flat]
    k1s, _k2s = so.gen_keys([nat[0], nat[-1], 12345, n - 1, nat[7]], n, prf,
                            seed=30)
    want = np.array([_core.eval_point_low(k1s[f >> depth], i, prf)
                     for f, i in zip(flat, nat)], dtype=np.uint64)
    keys_gpu = torch.from_numpy(np.stack(k1s)).to(_dev())
    out = torch.empty((batch, n), dtype=torch.int32, device=_dev())
    assert _hip.eval_slog(batch, depth, zlog) == 8
    _hip.eval_expand(keys_gpu.data_ptr(), out.data_ptr(), 0, batch, n, depth,
                     zlog, prf, _stream())
    pos = torch.tensor(flat, dtype=torch.int64, device=_dev())
    got = out.view(-1).index_select(0, pos).cpu().numpy().view(np.uint32)
    del out
    _release()
    bad = np.nonzero(got.astype(np.uint64) != want)[0]
    assert bad.size == 0, [hex(flat[i]) for i in bad[:8]]


def test_gpu_bfs_frontier_past_byte_2_32():
    """PEAK 15 to 27 GiB: batch 3 at n = 2^28 through eval_gpu.  The output
    is 3 GiB (key 2 starts at byte 2^31), the two frontiers 12 GiB (key 2's
    seeds of the last levels lie past byte 2^32).  The frontiers live in the
    launchers' grow-only scratch, which doubles from its earlier size and so
    may take up to twice that; it is kept for the rest of the process.  The
    breadth-first kernels read no table, so the engine gets a one-row
    placeholder instead of the 16 GiB table of this domain.  Positions are in
    natural order; S holds both leaves p and p + n/2 of a parent."""
    _need(27)
    prf = DPF.PRF_DUMMY
    depth, batch = 28, 3
    n = 1 << depth
    flat = so.shape_rows("bfs_b3_n28")
    assert {f >> depth for f in flat} == set(range(batch))
    assert any(f & (n >> 1) for f in flat) and any(
        not f & (n >> 1) for f in flat)
    k1s, _k2s = so.gen_keys([0, n - 1, (n >> 1) + 5], n, prf, seed=28)
    want = np.array([_core.eval_point_low(k1s[f >> depth], f & (n - 1), prf)
                     for f in flat], dtype=np.uint64)
    dpf = DPF(prf=prf)
    dpf._setup_domain(n, 16)
    dpf._table_gpu = torch.zeros((1, 16), dtype=torch.int32, device=_dev())
    out = dpf.eval_gpu(torch.from_numpy(np.stack(k1s)), one_hot_only=True,
                       strategy="bfs", out_device=True)
    assert out.shape == (batch, n) and out.is_contiguous()
    pos = torch.tensor(flat, dtype=torch.int64, device=_dev())
    got = out.reshape(-1).index_select(0, pos).cpu().numpy().view(np.uint32)
    del out
    dpf.eval_free()
    _release()
    bad = np.nonzero(got.astype(np.uint64) != want)[0]
    assert bad.size == 0, [hex(flat[i]) for i in bad[:8]]


def _ref_mod32(a, b):
    prod = a.astype(np.int64) @ b.astype(np.int64)
    return prod.astype(np.uint32).astype(np.int32)


def test_gpu_stream_gemm_b_past_2_32_elements():
    """PEAK 21 GiB: b [K, 68] with K = 2^26 + 65 is 18.3 GiB, 4.56e9
    elements; K % 4 = 1 takes the unaligned share loads, the last K segment
    is ragged, and N = 68 leaves a four-column tail behind the 16-column
    blocks.  a is zero except at the rows of S (first and last, around each
    boundary), at the last row of every K segment and the first of the next,
    and at seeded random rows; each of its three rows carries its own
    values.  The kernel does the same work whatever the data, so the
    expected result needs only those rows of b."""
    _need(21)
    M, K, N = 3, (1 << 26) + 65, 68
    segs, kchunk = _hip.gemm_u32_stream_split(M, K, N)
    assert segs > 1 and (segs - 1) * kchunk < K < segs * kchunk  # ragged
    assert K % 4 == 1 and N % 16 == 4
    rows = set(so.shape_rows("gemm_b"))
    assert min(rows) == 0 and max(rows) == K - 1
    for s in range(1, segs):
        rows.update((s * kchunk - 1, s * kchunk))
    rows = np.array(sorted(r for r in rows if 0 <= r < K), dtype=np.int64)

    dev = _dev()
    b = torch.empty((K, N), dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(68)
    step = 1 << 20
    for lo in range(0, K, step):
        hi = min(K, lo + step)
        b[lo:hi] = torch.randint(-(2**31), 2**31, (hi - lo, N),
                                 dtype=torch.int64, device=dev,
                                 generator=g).to(torch.int32)
    rng = np.random.default_rng(68)
    vals = so.random_rows(M, len(rows), seed=69)
    # each share row is nonzero on its own seeded part of the rows, on the
    # rows of S always
    keep = rng.integers(0, 4, (M, len(rows))) > 0
    keep |= np.isin(rows, so.shape_rows("gemm_b"))[None, :]
    vals = np.where(keep, vals, 0).astype(np.int32)
    a = torch.zeros((M, K), dtype=torch.int32, device=dev)
    rows_gpu = torch.from_numpy(rows).to(dev)
    a[:, rows_gpu] = torch.from_numpy(vals).to(dev)
    b_rows = b.index_select(0, rows_gpu).cpu().numpy()
    got = ops.pir_matmul_u32_stream(a, b).cpu().numpy()
    del a, b
    _release()
    assert np.array_equal(got, _ref_mod32(vals, b_rows))


def test_gpu_two_stage_end_to_end_past_2_32_elements(monkeypatch):
    """PEAK 22 GiB: n = 2^26 rows of 80 words (20 GiB, 5.4e9 elements)
    behind the default fused_words, so eval_gpu takes expand + stream GEMM,
    as shipped.  The row permutation is left on the host, as in the W=3
    test."""
    monkeypatch.setattr(DPF, "PERM_MATERIALIZE_MAX", 1 << 24)
    _need(22)
    prf = DPF.PRF_DUMMY
    st = _sparse("two_stage_n26_e80", 80, 80)
    dpf = _engine(prf, st)
    assert not dpf.fused_servable
    assert dpf._table_gpu.numel() * 4 > 2 * GIB  # past the MFMA dispatch
    _alphas, k1s, _k2s, want1, want2, secret = _case(prf, st)
    got = dpf.eval_gpu(_batch_of(k1s, 3)).numpy()
    assert got.shape == (3, 80)
    assert np.array_equal(got, want1[:3])
    assert np.array_equal(so.reconstruct(got, want2[:3]), secret[:3])
    dpf.eval_free()
    _release()
