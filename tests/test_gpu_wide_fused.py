"""Rows of up to 64 words in the fused kernel (DPF / BinnedDPF fused_words).

Every comparison is exact equality against eval_cpu: the arithmetic is mod
2^32, so there is no tolerance.  Tables are seeded full-range int32, so high
bits and wraparound are exercised and a swapped column block or row shows.

Geometry.  Depths 7..16 reach Z = 64 (one-wave reduction) and Z = 128, 256
(cross-wave reduction), DS = 1 (one leaf pair, no stack), DS = 2, the first
LDS stack level (depth 12) and a global-scratch level (depth 16).  Entry
sizes 17, 32, 33 and 64 are W = 2, 2, 3 and 4 column blocks, three of them
with padding columns that must come back trimmed.  Batch 1 takes the largest
j-split (every column combined by atomics); 1, 3 and 5 give odd unit counts,
so the AES K = 2 workgroups have a surplus unit.
"""

import functools

import numpy as np
import pytest
import torch

from gpudpf import BinnedDPF, DPF, _core

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

pytestmark = pytest.mark.gpu

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
DEPTHS = [7, 8, 9, 10, 12, 16]
ENTRIES = [17, 32, 33, 64]
BATCHES = [1, 3, 5]
N_KEYS = 5
GUARD = 0x5A5A5A5A


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


def _sub(a, b):
    return (a.to(torch.int64) - b.to(torch.int64)).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(prf, n, e, fused_words=64):
    """Per-shape fixture, built once and never modified: engine with the
    table resident, table, alphas, both servers' keys and CPU shares."""
    dpf = DPF(prf=prf, fused_words=fused_words)
    table = _rand((n, e), 1000 * e + n + prf)
    dpf.eval_init(table)
    rng = np.random.default_rng(n + e)
    alphas = [n - 1, 0] + [int(a) for a in rng.integers(1, n - 1, N_KEYS - 2)]
    k1s, k2s = dpf.gen_batch(alphas, n)
    cpu1, cpu2 = dpf.eval_cpu(k1s), dpf.eval_cpu(k2s)
    # the oracle itself reconstructs
    assert torch.equal(_sub(cpu1, cpu2), table[alphas])
    return dpf, table, alphas, k1s, k2s, cpu1, cpu2


def _check(prf, depth, e, batches=BATCHES):
    n = 1 << depth
    dpf, table, alphas, k1s, k2s, cpu1, cpu2 = _case(prf, n, e)
    ep = -(-e // 16) * 16
    assert dpf._depth == depth and dpf.fused_servable
    assert dpf._table_gpu.shape == (n, ep)
    for batch in batches:
        idx = [i % N_KEYS for i in range(batch)]
        a = dpf.eval_gpu(k1s[idx])
        b = dpf.eval_gpu(k2s[idx])
        assert a.shape == (batch, e) and a.dtype == torch.int32
        assert torch.equal(a, cpu1[idx]), (depth, e, batch)
        assert torch.equal(b, cpu2[idx]), (depth, e, batch)
        assert torch.equal(_sub(a, b), table[[alphas[i] for i in idx]])


@pytest.mark.parametrize("e", ENTRIES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_wide_matches_cpu(prf, depth, e, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _check(prf, depth, e)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("units", [1, 2, 3, 4])
def test_gpu_wide_aes_forced_units_are_clamped(units, depth, monkeypatch):
    aes = DPF.PRF_AES128
    zlog = _core.zlog_for_depth(depth)
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    for words in (32, 48, 64):   # unmeasured: the largest K allowed
        assert _hip.eval_units_per_wg(aes, 1000, words) == 2
    monkeypatch.setenv("GPUDPF_AES_UNITS", str(units))
    for batch in BATCHES:
        n_units = batch << _hip.eval_slog(batch, depth, zlog)
        for words in (32, 48, 64):
            assert _hip.eval_units_per_wg(aes, n_units, words) == min(units, 2)
        # 16-word rows keep the forced K
        assert _hip.eval_units_per_wg(aes, n_units, 16) == units
        assert _hip.eval_units_per_wg(aes, n_units) == units
        assert _hip.eval_units_per_wg(DPF.PRF_SALSA20, n_units, 64) == 1
    with pytest.raises(ValueError):
        _hip.eval_units_per_wg(aes, 1000, 24)
    for e in ENTRIES:
        _check(aes, depth, e)


@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_wide_one_segment_per_key(prf, monkeypatch):
    """Batch 1025 at depth 7: slog = 0, one unit per key, 1025 units (odd)."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    assert _hip.eval_slog(1025, 7, _core.zlog_for_depth(7)) == 0
    for e in (33, 64):
        _check(prf, 7, e, batches=[1025])


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_wide_non_power_of_two_rows(prf, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    n, e = 300, 33
    dpf, table, alphas, k1s, k2s, cpu1, cpu2 = _case(prf, n, e)
    assert dpf._n_domain == 512 and dpf._table_gpu.shape == (512, 48)
    a, b = dpf.eval_gpu(k1s), dpf.eval_gpu(k2s)
    assert torch.equal(a, cpu1) and torch.equal(b, cpu2)
    assert torch.equal(_sub(a, b), table[alphas])


# ---------------------------------------------------------------------------
# The same table behind two instances: default (two-stage) and wide (fused)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_SALSA20],
                         ids=PRF_IDS.get)
def test_gpu_wide_and_two_stage_agree(prf, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    n, e = 1 << 10, 33
    wide, table, _alphas, k1s, _k2s, cpu1, _c2 = _case(prf, n, e)
    default = DPF(prf=prf)
    default.eval_init(table)
    assert not default.fused_servable and wide.fused_servable
    got_default = default.eval_gpu(k1s)              # two-stage
    assert torch.equal(got_default, cpu1)
    assert torch.equal(wide.eval_gpu(k1s), got_default)
    assert torch.equal(wide.eval_gpu(k1s, strategy="two_stage"), cpu1)
    # the coop kernel stays 16-word: refused, not launched on wide rows
    with pytest.raises(Exception, match="coop"):
        wide.eval_gpu(k1s[:1], strategy="coop")
    # wider than the instance's limit: two-stage, as before
    dpf65, _t, _a, k65, _k2, cpu65, _c = _case(prf, n, 65)
    assert dpf65._entry_padded == 80 and not dpf65.fused_servable
    assert torch.equal(dpf65.eval_gpu(k65), cpu65)
    # a narrower limit than the table: two-stage again
    dpf32, _t, _a, k32, _k2, cpu32, _c = _case(prf, n, e, fused_words=32)
    assert not dpf32.fused_servable
    assert torch.equal(dpf32.eval_gpu(k32), cpu32)


# ---------------------------------------------------------------------------
# Binned: 3 bins of unequal size, keys hitting bins 0, 1, 2 in mixed order
# (a block-stride bug only shows for bin >= 1; the last bin ends the table)
# ---------------------------------------------------------------------------
KEY_BINS = [2, 0, 1, 2, 0, 2, 1]


@functools.lru_cache(maxsize=None)
def _binned_case(prf, sizes, e):
    tabs = [_rand((nb, e), 77 * e + 13 * b + prf) for b, nb in enumerate(sizes)]
    dpf = BinnedDPF(prf=prf, fused_words=64)
    dpf.eval_init(tabs)
    rng = np.random.default_rng(e + sizes[0])
    rows = [sizes[2] - 1, 0, 0, int(rng.integers(0, sizes[2])), sizes[0] - 1,
            0, 0]
    k1s, k2s = dpf.gen_batch(rows, KEY_BINS)
    cpu1, cpu2 = dpf.eval_cpu(k1s, KEY_BINS), dpf.eval_cpu(k2s, KEY_BINS)
    want = torch.stack([tabs[b][r] for r, b in zip(rows, KEY_BINS)])
    assert torch.equal(_sub(cpu1, cpu2), want)
    # the oracle tells the bins apart
    wrong = dpf.eval_cpu(k1s[:1], [0])
    assert not torch.equal(wrong[0], cpu1[0])
    return dpf, want, k1s, k2s, cpu1, cpu2


@pytest.mark.parametrize("e", [40, 64])
@pytest.mark.parametrize("sizes", [(200, 1, 129), (4096, 1, 2500)],
                         ids=["depth8", "depth12"])
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_wide_binned_matches_cpu(prf, sizes, e, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    monkeypatch.delenv("GPUDPF_DEBUG", raising=False)
    dpf, want, k1s, k2s, cpu1, cpu2 = _binned_case(prf, sizes, e)
    ep = -(-e // 16) * 16
    assert dpf._table_gpu.shape == (3, dpf._n_domain, ep)
    for b in range(3):
        assert torch.equal(dpf._table_gpu[b].cpu(), dpf.bin_block(b)), b
    a = dpf.eval_gpu(k1s, KEY_BINS)
    b = dpf.eval_gpu(k2s, torch.tensor(KEY_BINS, dtype=torch.int64))
    assert a.shape == (len(KEY_BINS), e)
    assert torch.equal(a, cpu1) and torch.equal(b, cpu2)
    assert torch.equal(_sub(a, b), want)
    assert dpf._plan is None
    # the bound plan and the zero-copy path
    dev = dpf._table_gpu.device
    dpf.bind_bins(KEY_BINS)
    try:
        out = torch.full((len(KEY_BINS), ep), 7, dtype=torch.int32, device=dev)
        dpf.eval_gpu_into(k2s.to(dev), out)
        assert torch.equal(out[:, :e].cpu(), cpu2)
        assert not out[:, e:].any()
    finally:
        dpf._plan = None   # the fixture is shared


# ---------------------------------------------------------------------------
# Servers
# ---------------------------------------------------------------------------
def _three_batches(k1s, k2s, cpu1, cpu2, order2):
    return [(k1s, cpu1), (k2s, cpu2), (k1s[order2], cpu1[order2])]


def _serve_all(graphed, piped, batches, e):
    for keys, cpu in batches:
        got = graphed.eval(keys)
        assert got.shape == cpu.shape and got.shape[1] == e
        assert torch.equal(got, cpu)
    h0 = piped.submit(batches[0][0])
    h1 = piped.submit(batches[1][0])       # two in flight before collecting
    assert torch.equal(piped.collect(h0), batches[0][1])
    h2 = piped.submit(batches[2][0])
    assert torch.equal(piped.collect(h1), batches[1][1])
    got = piped.collect(h2)
    assert got.shape[1] == e and torch.equal(got, batches[2][1])


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_SALSA20],
                         ids=PRF_IDS.get)
def test_gpu_servers_serve_wide_dpf(prf, monkeypatch):
    from gpudpf.serving import (GraphedServer, PipelinedServer,
                                TwoStageServer)

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    e = 33
    dpf, _t, _a, k1s, k2s, cpu1, cpu2 = _case(prf, 1 << 16, e)
    assert dpf._scratch_bytes(N_KEYS) > 0  # the slots own real scratch
    graphed = GraphedServer(dpf, batch=N_KEYS)
    assert not graphed.wide
    piped = PipelinedServer(dpf, batch=N_KEYS, depth=2)
    _serve_all(graphed, piped,
               _three_batches(k1s, k2s, cpu1, cpu2, [4, 3, 2, 1, 0]), e)
    # the refusals name the instance's limit, not 16
    with pytest.raises(Exception, match=r"wide entries \(> 64 words\)"):
        TwoStageServer(dpf, batch=N_KEYS)
    dpf65 = _case(prf, 1 << 10, 65)[0]
    with pytest.raises(Exception, match=r"fused path \(entry <= 64 words\)"):
        PipelinedServer(dpf65, batch=N_KEYS)


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_SALSA20],
                         ids=PRF_IDS.get)
def test_gpu_servers_serve_wide_binned(prf, monkeypatch):
    from gpudpf.serving import GraphedServer, PipelinedServer

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    e = 40
    dpf, _want, k1s, k2s, cpu1, cpu2 = _binned_case(prf, (4096, 1, 2500), e)
    dpf.bind_bins(KEY_BINS)
    try:
        graphed = GraphedServer(dpf, batch=len(KEY_BINS))
        piped = PipelinedServer(dpf, batch=len(KEY_BINS), depth=2)
        # a second order that keeps every slot's bin: swap equal-bin keys
        order2 = [5, 4, 6, 0, 1, 3, 2]
        assert [KEY_BINS[i] for i in order2] == KEY_BINS
        _serve_all(graphed, piped,
                   _three_batches(k1s, k2s, cpu1, cpu2, order2), e)
    finally:
        dpf._plan = None


def test_gpu_default_instance_refusals_are_unchanged():
    from gpudpf.serving import (GraphedServer, PipelinedServer,
                                TwoStageServer)

    prf, n, e = DPF.PRF_SALSA20, 1 << 10, 32
    table = _rand((n, e), 5)
    dpf = DPF(prf=prf)
    dpf.eval_init(table)
    keys, _ = dpf.gen_batch([1, 2, 3], n)
    with pytest.raises(Exception, match=r"fused path \(entry <= 16 words\)"):
        PipelinedServer(dpf, batch=3)
    assert GraphedServer(dpf, batch=3).wide
    srv = TwoStageServer(dpf, batch=3)
    assert torch.equal(srv.collect(srv.submit(keys)), dpf.eval_cpu(keys))
    binned = BinnedDPF(prf=prf)
    with pytest.raises(Exception, match="at most 16"):
        binned.eval_init([table])


# ---------------------------------------------------------------------------
# Launch checks: nothing is launched (the output keeps its guard pattern)
# ---------------------------------------------------------------------------
def test_gpu_wide_launch_checks_launch_nothing(monkeypatch):
    monkeypatch.delenv("GPUDPF_DEBUG", raising=False)
    prf, n, e, b = DPF.PRF_SALSA20, 1 << 10, 33, 3
    dpf, _t, _a, k1s, _k2, cpu1, _c = _case(prf, n, e)
    dev = dpf._table_gpu.device
    keys_gpu = k1s[:b].to(dev)
    out16 = torch.full((b, 16), GUARD, dtype=torch.int32, device=dev)
    out48 = torch.full((b, 48), GUARD, dtype=torch.int32, device=dev)
    with pytest.raises(Exception, match="^out must be"):
        dpf._launch_fused(keys_gpu, out16)
    with pytest.raises(Exception, match="^out must be"):
        dpf._launch_fused(keys_gpu, torch.full(
            (b, 64), GUARD, dtype=torch.int32, device=dev))
    stream = torch.cuda.current_stream(dev).cuda_stream
    for words in (24, 0, 80, -16):
        with pytest.raises(ValueError):
            _hip.eval_fused(keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(),
                            out48.data_ptr(), dpf._aes_ptr, b, n, dpf._depth,
                            dpf._zlog, prf, stream, entry_words=words)
        with pytest.raises(ValueError):
            _hip.eval_fused_binned(
                keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(),
                keys_gpu.data_ptr(), out48.data_ptr(), dpf._aes_ptr, b, n,
                dpf._depth, dpf._zlog, 1, prf, stream, entry_words=words)
    # a table wider than the instance serves fused
    narrow = _case(prf, n, e, fused_words=32)[0]
    with pytest.raises(Exception, match="fused_words"):
        narrow._launch_fused(keys_gpu, out48)
    with pytest.raises(Exception, match="fused_words"):
        narrow._launch_fused(keys_gpu, out16)
    with pytest.raises(Exception, match="fused_words"):
        narrow.eval_gpu_into(keys_gpu, torch.full(
            (b, 32), GUARD, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    assert bool((out16 == GUARD).all().item())
    assert bool((out48 == GUARD).all().item())
    # and the correct launch after all of them is exact
    out48.zero_()
    dpf._launch_fused(keys_gpu, out48)
    assert torch.equal(out48[:, :e].cpu(), cpu1[:b])
    assert not out48[:, e:].any()


# ---------------------------------------------------------------------------
# pir.serve: a collocated plan with 48-word rows, served and decoded
# ---------------------------------------------------------------------------
def test_gpu_serve_round_trip_wide():
    from gpudpf.serving import PipelinedServer
    from pir import serve
    from test_wide_fused_cpu import (wide_plan, wide_requests,
                                     wide_round_trip)

    opt, table, pats = wide_plan()
    dpf = BinnedDPF(prf=DPF.PRF_CHACHA20, fused_words=64)
    dpf.eval_init(serve.bin_tables(opt, table, max_words=64))
    assert dpf._entry_padded == 48
    bins = serve.slot_bins(opt)
    dpf.bind_bins(bins)
    piped = PipelinedServer(dpf, batch=len(bins))

    def shares(keys):
        got = piped.collect(piped.submit(keys))
        assert got.shape == (len(bins), 48)
        assert torch.equal(got, dpf.eval_cpu(keys, bins))
        return got

    n_rec = sum(len(wide_round_trip(opt, table, dpf, idx, shares))
                for idx in wide_requests(opt, pats))
    assert n_rec > 0
