"""The packed kernels (LANES = 4 of dpf_eval_kernel) on the GPU.

A packed engine over n rows walks a tree of depth D = log2(n) - 2, so the
launch geometry (DS = D - zlog, slog, scratch) is that of a plain launch at
depth D; what is new is the leaf step: 8 shares per pair, 8 consecutive
rows of the packed row order, four lane blocks into one set of sums.

Every comparison is exact: one server's GPU shares against the CPU core for
the same keys (reconstruction alone cancels what both servers get equally
wrong), plus reconstruction from a GPU share and a CPU share.
"""

import functools
import gc

import numpy as np
import pytest
import torch

import packed_oracle as po
import sparse_oracle as so
from gpudpf import DPF, PackedDPF, _core

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

pytestmark = pytest.mark.gpu

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
N_KEYS = 7                    # coprime to every K = 2, 3, 4
# tree depth -> DS: no stack, each register level, the first LDS level, the
# grown shared slice, the first and the fifth global level
DEPTH_DS = {7: 1, 10: 2, 11: 3, 12: 4, 14: 6, 16: 8, 20: 12}
DEPTHS = sorted(DEPTH_DS)
EXPAND_MAX_BYTES = 256 << 20
PACKED_AES_MAX_UNITS = 3      # K = 4 spills on gfx950 (docs/KERNEL_NOTES.md)
GUARD = 0x5A5A5A5A
GUARD_WORDS = 4096
GIB = 1 << 30


def _points(D):
    """(batch, slog): batch 3 reaches the depth's slog cap min(DS - 2, 8);
    depths <= 12 also run slog 0 (batch 1025) and batch 129, which splits 8
    ways where the cap allows."""
    cap = max(0, min(DEPTH_DS[D] - 2, 8))
    pts = [(3, cap)]
    if D <= 12:
        pts += [(1025, 0), (129, min(3, cap))]
    return pts


def _check_slog(batch, D, slog):
    zlog = _core.zlog_for_depth(D)
    assert D - zlog == DEPTH_DS[D]
    assert _hip.eval_slog(batch, D, zlog) == slog, (D, batch)


@functools.lru_cache(maxsize=None)
def _table(n, e=16):
    g = torch.Generator().manual_seed(9000 + n.bit_length() * 100 + e)
    return torch.randint(-(2**31), 2**31, (n, e), dtype=torch.int64,
                         generator=g).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(prf, D, e=16):
    """Per-(prf, D, e) fixture, built once and never modified: engine with
    the table resident, N_KEYS key pairs (alphas distinct, one per lane
    among them) and the CPU shares of both servers."""
    n = 4 << D
    table = _table(n, e)
    alphas = po.lane_alphas(n, N_KEYS, seed=prf * 100 + D)
    k1n, k2n = po.gen_keys(alphas, n, prf, seed=prf * 1000 + D)
    k1s = [torch.from_numpy(k) for k in k1n]
    k2s = [torch.from_numpy(k) for k in k2n]
    dpf = PackedDPF(prf=prf)
    dpf.eval_init(table)
    assert (dpf._depth, dpf._n_domain) == (D, n)
    tnp = table.numpy()
    cpu1 = np.stack([_core.eval_fused_cpu(k, tnp, prf) for k in k1n])
    cpu2 = np.stack([_core.eval_fused_cpu(k, tnp, prf) for k in k2n])
    if D <= 12:  # the engine's own CPU path agrees
        assert np.array_equal(cpu1, dpf.eval_cpu(k1s).numpy())
    assert np.array_equal(so.reconstruct(cpu1, cpu2),
                          table.numpy()[alphas])  # the oracle itself
    return dpf, alphas, k1s, k2s, cpu1, cpu2


def _batch_of(keys, batch):
    return torch.stack([keys[i % len(keys)] for i in range(batch)])


def _check_fused(prf, D):
    dpf, alphas, k1s, k2s, cpu1, cpu2 = _case(prf, D)
    secret = _table(4 << D).numpy()[alphas]
    for batch, slog in _points(D):
        _check_slog(batch, D, slog)
        idx = np.arange(batch) % N_KEYS
        a = dpf.eval_gpu(_batch_of(k1s, batch)).numpy()
        b = dpf.eval_gpu(_batch_of(k2s, batch)).numpy()
        assert np.array_equal(a, cpu1[idx]), (D, batch)
        assert np.array_equal(b, cpu2[idx]), (D, batch)
        assert np.array_equal(so.reconstruct(a, cpu2[idx]), secret[idx])


# ---------------------------------------------------------------------------
# Geometry lattice
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_packed_fused_matches_cpu(prf, D, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _check_fused(prf, D)


@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_packed_expand_matches_cpu(prf, D, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    dpf, _alphas, k1s, k2s, _c1, _c2 = _case(prf, D)
    n = 4 << D
    pts = [(b, s) for b, s in _points(D) if b * n * 4 <= EXPAND_MAX_BYTES]
    assert len(_points(D)) - len(pts) == 0  # largest: 3 x 2^22 x 4 B = 48 MiB
    for keys in (k1s, k2s):
        want = np.stack([_core.expand(k.numpy(), prf) for k in keys])
        for batch, slog in pts:
            _check_slog(batch, D, slog)
            got = dpf.eval_gpu(_batch_of(keys, batch),
                               one_hot_only=True).numpy()
            assert got.shape == (batch, n)
            assert np.array_equal(got, want[np.arange(batch) % N_KEYS]), \
                (D, batch)


def _guarded(words, device):
    return torch.full((words + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32,
                      device=device)


def _guards_intact(big, words):
    return bool((big[:GUARD_WORDS] == GUARD).all().item()) and \
        bool((big[GUARD_WORDS + words:] == GUARD).all().item())


@pytest.mark.parametrize("D", [7, 12, 16])
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_packed_raw_launches_stay_in_bounds(prf, D, monkeypatch):
    """The raw expand output (rows in packed order) and the fused output in
    buffers of exactly their size, and at D = 16 the sibling stack in a
    caller-owned buffer of exactly eval_scratch_bytes, all carved from
    tensors whose head and tail hold a pattern."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    dpf, _alphas, k1s, _k2s, cpu1, _c2 = _case(prf, D)
    n, zlog, batch = 4 << D, dpf._zlog, 3
    dev = dpf._table_gpu.device
    keys_gpu = _batch_of(k1s, batch).to(dev).contiguous()
    need = dpf._scratch_bytes(batch)
    slog = _hip.eval_slog(batch, D, zlog)
    assert need == (batch << slog) * max(0, D - zlog - 7) * (1 << zlog) * 16
    assert (need > 0) == (D == 16)
    perm = _core.packed_perm_table(n, zlog)
    want = np.empty((batch, n), dtype=np.int32)
    for i in range(batch):
        want[i, perm] = _core.expand(k1s[i].numpy(), prf)

    for own in ([False, True] if need else [False]):
        scratch = _guarded(need // 4, dev) if own else None
        carved = None if scratch is None else \
            scratch[GUARD_WORDS:GUARD_WORDS + need // 4].view(torch.uint8)
        out = _guarded(batch * n, dev)
        shares = out[GUARD_WORDS:GUARD_WORDS + batch * n].view(batch, n)
        dpf._launch_expand(keys_gpu, shares, scratch=carved)
        torch.cuda.synchronize(dev)
        assert np.array_equal(shares.cpu().numpy(), want), (D, own)
        assert _guards_intact(out, batch * n)
        fout = _guarded(batch * 16, dev)
        fused = fout[GUARD_WORDS:GUARD_WORDS + batch * 16].view(batch, 16)
        fused.zero_()
        dpf._launch_fused(keys_gpu, fused, scratch=carved)
        torch.cuda.synchronize(dev)
        assert np.array_equal(fused.cpu().numpy(), cpu1[:batch]), (D, own)
        assert _guards_intact(fout, batch * 16)
        if own:
            assert _guards_intact(scratch, need // 4)
            with pytest.raises(ValueError):  # one byte short: no launch
                _hip.eval_fused_packed(
                    keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(),
                    fused.data_ptr(), dpf._aes_ptr, batch, n, D, zlog, prf,
                    torch.cuda.current_stream(dev).cuda_stream,
                    carved.data_ptr(), need - 1)


# ---------------------------------------------------------------------------
# AES units per workgroup
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [12, 16])
@pytest.mark.parametrize("units", [1, 2, 3, 4])
def test_gpu_packed_aes_units(units, D, monkeypatch):
    """Every K the build has, forced; a forced K above the cap is clamped
    to it."""
    monkeypatch.setenv("GPUDPF_AES_UNITS", str(units))
    prf = DPF.PRF_AES128
    for n_units in (7, 768, 1000):
        assert _hip.eval_units_per_wg(prf, n_units, 16, lanes=4) \
            == min(units, PACKED_AES_MAX_UNITS)
    assert _hip.eval_units_per_wg(prf, 1000) == units  # plain: unchanged
    dpf, _alphas, k1s, k2s, cpu1, cpu2 = _case(prf, D)
    assert np.array_equal(dpf.eval_gpu(k1s).numpy(), cpu1)
    assert np.array_equal(dpf.eval_gpu(k2s).numpy(), cpu2)
    want = _core.expand(k1s[3].numpy(), prf)
    got = dpf.eval_gpu(k1s, one_hot_only=True).numpy()
    assert np.array_equal(got[3], want)


def test_gpu_packed_aes_units_default(monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    for n_units in (1, 256, 2048):
        assert _hip.eval_units_per_wg(DPF.PRF_AES128, n_units, 16, lanes=4) \
            == PACKED_AES_MAX_UNITS


# ---------------------------------------------------------------------------
# Servers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prf", [DPF.PRF_CHACHA20, DPF.PRF_AES128],
                         ids=PRF_IDS.get)
def test_gpu_servers_serve_packed(prf, monkeypatch):
    from gpudpf.serving import GraphedServer, PipelinedServer

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    D, batch = 16, 5
    dpf, _alphas, k1s, k2s, cpu1, cpu2 = _case(prf, D)
    assert dpf._scratch_bytes(batch) > 0  # the slots own real scratch
    ka, kb = torch.stack(k1s[:batch]), torch.stack(k2s[2:2 + batch])
    wa, wb = torch.from_numpy(cpu1[:batch]), torch.from_numpy(cpu2[2:2 + batch])
    graphed = GraphedServer(dpf, batch=batch)
    assert not graphed.wide
    assert torch.equal(graphed.eval(ka), wa)
    assert torch.equal(graphed.eval(kb), wb)
    piped = PipelinedServer(dpf, batch=batch, depth=2)
    h0 = piped.submit(ka)
    h1 = piped.submit(kb)            # two in flight before either is collected
    assert torch.equal(piped.collect(h0), wa)
    h2 = piped.submit(ka)
    assert torch.equal(piped.collect(h1), wb)
    assert torch.equal(piped.collect(h2), wa)
    # the zero-copy path
    dev = dpf._table_gpu.device
    out = torch.full((batch, 16), 7, dtype=torch.int32, device=dev)
    dpf.eval_gpu_into(kb.to(dev), out)
    assert torch.equal(out.cpu(), wb)


# ---------------------------------------------------------------------------
# Two-stage: entries wider than 16 words
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_packed_two_stage(prf, monkeypatch):
    from gpudpf.serving import GraphedServer, PipelinedServer, TwoStageServer

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    D, e = 10, 24
    dpf, alphas, k1s, k2s, cpu1, cpu2 = _case(prf, D, e)
    assert dpf._entry_padded == 32 and not dpf.fused_servable
    table = _table(4 << D, e).numpy()
    for batch in (5, 130):  # the stream GEMM, then the MFMA one
        idx = np.arange(batch) % N_KEYS
        a = dpf.eval_gpu(_batch_of(k1s, batch)).numpy()
        assert a.shape == (batch, e)
        assert np.array_equal(a, cpu1[idx]), batch
        b = dpf.eval_gpu(_batch_of(k2s, batch)).numpy()
        assert np.array_equal(b, cpu2[idx]), batch
        assert np.array_equal(so.reconstruct(a, cpu2[idx]),
                              table[np.asarray(alphas)[idx]])
    with pytest.raises(Exception, match="wider than the 16"):
        dpf._launch_fused(torch.stack(k1s).to(dpf._table_gpu.device),
                          torch.zeros((N_KEYS, 32), dtype=torch.int32,
                                      device=dpf._table_gpu.device))
    with pytest.raises(Exception, match="fused path"):
        PipelinedServer(dpf, batch=5)
    keys = torch.stack(k1s[:5])
    want = torch.from_numpy(cpu1[:5])
    graphed = GraphedServer(dpf, batch=5)
    assert graphed.wide and torch.equal(graphed.eval(keys), want)
    srv = TwoStageServer(dpf, batch=5)
    assert torch.equal(srv.collect(srv.submit(keys)), want)


# ---------------------------------------------------------------------------
# Ingest
# ---------------------------------------------------------------------------
def test_gpu_packed_ingest(monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    prf, n, e = DPF.PRF_SALSA20, 5000, 7   # domain 8192, tree depth 11
    dense = torch.zeros((n, e), dtype=torch.int32)
    q = 8192 // 4
    idx = [0, 4999, q - 1, q, q + 77, 2 * q - 1, 2 * q, 2 * q + 5, 17, 4500]
    assert len(set(idx)) == len(idx)
    assert {i // q for i in idx} == {0, 1, 2}  # 5000 rows end inside lane 2
    rows = torch.from_numpy(so.random_rows(len(idx), e, seed=3))
    dense[idx] = rows
    dpf = PackedDPF(prf=prf)
    dpf.eval_init_empty(n, e)
    assert (dpf._n_domain, dpf._depth, dpf._zlog) == (8192, 11, 8)
    dpf.table_write(torch.tensor(idx), rows)
    assert torch.equal(dpf.table_read(idx).cpu(), rows)
    # they landed where the Python permutation says, and nowhere else
    prow = [po.packed_perm(i, 11, 8) for i in idx]
    dev = dpf._table_gpu.device
    assert torch.equal(dpf._table_gpu[torch.tensor(prow, device=dev), :e].cpu(),
                       rows)
    assert int((dpf._table_gpu != 0).any(dim=1).sum()) == len(idx)
    ref = PackedDPF(prf=prf, device="cpu")
    ref.eval_init(dense)
    k1s, k2s = ref.gen_batch(idx[:6] + [1, 2], n)
    a = dpf.eval_gpu(k1s)
    assert torch.equal(a, ref.eval_cpu(k1s))
    assert torch.equal(dpf.eval_gpu(k2s), ref.eval_cpu(k2s))
    assert torch.equal(
        torch.from_numpy(so.reconstruct(a.numpy(), ref.eval_cpu(k2s).numpy())),
        dense[idx[:6] + [1, 2]])
    # a full lane 3 too: the whole domain
    full = PackedDPF(prf=prf)
    full.eval_init_empty(8192, e)
    full.table_write([8191, 3 * q], rows[:2])
    assert torch.equal(full.table_read([3 * q, 8191]).cpu(), rows[[1, 0]])


# ---------------------------------------------------------------------------
# Refusals that need the device state
# ---------------------------------------------------------------------------
def test_gpu_engines_refuse_each_others_keys():
    dpf, _alphas, k1s, _k2s, _c1, _c2 = _case(DPF.PRF_DUMMY, 10)
    n = 4 << 10
    plain = DPF(prf=DPF.PRF_DUMMY)
    plain.eval_init(_table(n))
    pk, _ = plain.gen(5, n)
    with pytest.raises(Exception, match="packed keys"):
        dpf.eval_gpu([pk])
    with pytest.raises(Exception, match="plain keys"):
        plain.eval_gpu([k1s[0]])
    with pytest.raises(Exception, match="mixed"):
        dpf.eval_gpu([k1s[0], pk])
    for strategy in ("bfs", "coop"):
        with pytest.raises(NotImplementedError, match="fused"):
            dpf.eval_gpu([k1s[0]], strategy=strategy)


# ---------------------------------------------------------------------------
# Large offsets: an 8 GiB table
# ---------------------------------------------------------------------------
def _need(peak_gib):
    """Skip only when the device cannot hold the test's peak plus 4 GiB."""
    gc.collect()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    if free < (peak_gib + 4) * GIB:
        pytest.skip("needs %d GiB of free device memory (peak %d GiB + 4), "
                    "%.1f GiB free" % (peak_gib + 4, peak_gib, free / GIB))


@functools.lru_cache(maxsize=None)
def _large():
    return po.PackedSparseTable(po.LARGE_D, 16, po.LARGE_WORDS, seed=2500,
                                flat_rows=tuple(po.large_rows()))


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_packed_large_offsets(prf, monkeypatch):
    """PEAK 8 GiB: 2^27 rows of 16 words, tree depth 25.  The table crosses
    bytes 2^31 and 2^32 and ends at element 2^31; it is zero except the rows
    S (test_packed_cpu.py proves where they lie), and one server's share is
    compared with the sum over S of eval_point_low * row."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _need(8)
    st = _large()
    n_keys = 5
    alphas = st.alphas(n_keys)
    assert len(alphas) == n_keys
    k1s, k2s = po.gen_keys(alphas, st.n, prf, seed=prf * 1000 + st.D)
    want1 = np.stack([st.share(k, prf) for k in k1s])
    want2 = np.stack([st.share(k, prf) for k in k2s])
    secret = np.stack([st.row_of(a) for a in alphas])
    assert np.array_equal(so.reconstruct(want1, want2), secret)  # the oracle
    dpf = PackedDPF(prf=prf)
    dpf.PERM_MATERIALIZE_MAX = 1 << 26  # rows through packed_perm_rows
    dpf.eval_init_empty(st.n, st.e)
    assert (dpf._depth, dpf._zlog, dpf._perm_gpu) == (25, 8, None)
    assert dpf._table_gpu.numel() * 4 == 8 * GIB
    nat = torch.from_numpy(st.nat)
    dpf.table_write(nat, torch.from_numpy(st.rows))
    assert np.array_equal(dpf.table_read(nat).cpu().numpy(), st.rows)
    prow = torch.tensor(st.prow, dtype=torch.int64,
                        device=dpf._table_gpu.device)
    assert np.array_equal(dpf._table_gpu[prow].cpu().numpy(), st.rows)
    assert _hip.eval_slog(n_keys, 25, 8) == 8
    assert dpf._scratch_bytes(n_keys) == (n_keys << 8) * 10 * 256 * 16
    got = dpf.eval_gpu(torch.from_numpy(np.stack(k1s))).numpy()
    assert np.array_equal(got, want1)
    assert np.array_equal(so.reconstruct(got, want2), secret)
    dpf.eval_free()
    del dpf, prow
    gc.collect()
    torch.cuda.empty_cache()
