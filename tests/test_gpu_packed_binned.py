"""The packed binned fused kernel (gpudpf.PackedBinnedDPF) on the GPU.

A packed binned engine over bins of n = 4 << D rows walks a tree of depth D
per key, so the launch geometry (DS = D - zlog, slog, scratch) is the plain
binned kernel's at depth D; what is new is the leaf step against a bin block:
8 shares per pair, 8 consecutive rows of 16 * W words in packed order,
4 * W blocks of 16 words into W sets of sums.

Geometry: tree depths 7, 9, 11 and 16 are Z = 64 with DS 1; Z = 256 with
DS 1; DS 3, the first j-split; DS 8 with one sibling-stack level in global
scratch.  Every lattice run holds 5 bins of unequal size and 7 distinct
(key, bin) pairs with bins [4, 0, 2, 2, 4, 1, 3], replicated i % 7 to batches
3, 65 and 1025, so units of different bins share a workgroup (AES K > 1).

All comparisons are exact: one server's GPU shares against
_core.eval_fused_cpu(key, that key's own zero-padded natural-order bin
table), plus reconstruction from one GPU and one CPU share.  The bin tables
are independently random; the fixtures assert on the CPU that each key's
share against its own bin differs from its share against bin 0.
"""

import functools
import gc

import numpy as np
import pytest
import torch

import packed_binned_oracle as pbo
import packed_oracle as po
import sparse_oracle as so
from gpudpf import DPF, PackedBinnedDPF, PackedDPF, _core
from pir import serve

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

pytestmark = pytest.mark.gpu

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
DEPTHS = [7, 9, 11, 16]       # tree depths D; bin domains 4 << D
BATCHES = [3, 65, 1025]
# eval_slog(batch, D): the largest s <= min(DS - 2, 8) with batch << s <= 2048
SLOG = {7: [0, 0, 0], 9: [0, 0, 0], 11: [1, 1, 0], 16: [6, 4, 0]}
KEY_BINS = [4, 0, 2, 2, 4, 1, 3]
N_KEYS = len(KEY_BINS)
WIDE_BINS = [2, 0, 1, 2, 0]
GUARD = 0x5A5A5A5A
GUARD_WORDS = 4096
GIB = 1 << 30


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


def _padded(t, n, words):
    p = np.zeros((n, words), dtype=np.int32)
    p[: t.shape[0], : t.shape[1]] = t.numpy()
    return p


def _words(e):
    return -(-e // 16) * 16


def _sizes(D):
    n = 4 << D
    # a one-row bin, two that need padding, two that fill the domain; the
    # last bin is full, so its rows end where the device table ends
    return [n, 1, n // 2 + 13, n - 3, n]


def _wide_sizes(D):
    n = 4 << D
    return [n, 1, n // 2 + 13]


@functools.lru_cache(maxsize=None)
def _tables(D, e=16):
    sizes = _sizes(D) if e == 16 else _wide_sizes(D)
    return tuple(_rand((nb, e), 1000 * D + 10 * e + b)
                 for b, nb in enumerate(sizes))


def _engine(prf, D, e=16):
    d = PackedBinnedDPF(prf=prf, fused_words=_words(e))
    tabs = _tables(D, e)
    d.eval_init(list(tabs))
    assert (d._depth, d._n_domain) == (D, 4 << D)
    assert d._zlog == _core.zlog_for_depth(D) == min(8, D - 1)
    assert d._table_gpu.shape == (len(tabs), 4 << D, _words(e))
    return d


def _keys_and_shares(prf, D, e, rows, bins):
    """Seeded packed key pairs for rows[i] of bins[i] and both servers' CPU
    shares against each key's own padded bin table; asserts that the oracle
    reconstructs and tells the bins apart."""
    n = 4 << D
    tabs = _tables(D, e)
    k1n, k2n = po.gen_keys(rows, n, prf, seed=prf * 1000 + D * 10 + e)
    pad = [_padded(t, n, _words(e)) for t in tabs]
    cpu1 = np.stack([_core.eval_fused_cpu(k, pad[b], prf)
                     for k, b in zip(k1n, bins)])
    cpu2 = np.stack([_core.eval_fused_cpu(k, pad[b], prf)
                     for k, b in zip(k2n, bins)])
    want = np.stack([pad[b][r] for r, b in zip(rows, bins)])
    assert np.array_equal(so.reconstruct(cpu1, cpu2), want)
    for i, b in enumerate(bins):
        if b != 0:
            wrong = _core.eval_fused_cpu(k1n[i], pad[0], prf)
            assert not np.array_equal(wrong, cpu1[i]), i
    k1s = [torch.from_numpy(k) for k in k1n]
    k2s = [torch.from_numpy(k) for k in k2n]
    return want, k1s, k2s, cpu1, cpu2


@functools.lru_cache(maxsize=None)
def _case(prf, D):
    """Per-(prf, D) lattice fixture, built once and never modified (eval_gpu
    leaves the engine as it is): engine, secret rows, 7 key pairs, CPU
    shares."""
    n, q = 4 << D, (4 << D) // 4
    sizes = _sizes(D)
    rng = np.random.default_rng(prf * 100 + D)
    rows = [n - 1, 0, int(rng.integers(q, 2 * q)), sizes[2] - 1,
            int(rng.integers(2 * q, 3 * q)), 0,
            int(rng.integers(3 * q, sizes[3]))]
    assert all(r < sizes[b] for r, b in zip(rows, KEY_BINS))
    assert rows[3] == n // 2 + 12             # the last row of bin 2
    assert {r // q for r in rows} == {0, 1, 2, 3}   # an alpha in every lane
    return (_engine(prf, D),) + _keys_and_shares(prf, D, 16, rows, KEY_BINS)


@functools.lru_cache(maxsize=None)
def _wide_case(prf, D, e):
    """The same for three unequal bins of e-word entries and 5 keys."""
    n, q = 4 << D, (4 << D) // 4
    sizes = _wide_sizes(D)
    rng = np.random.default_rng(prf * 100 + D + 7 * e)
    rows = [sizes[2] - 1, n - 1, 0, int(rng.integers(q, 2 * q)),
            int(rng.integers(3 * q, n))]
    assert all(r < sizes[b] for r, b in zip(rows, WIDE_BINS))
    assert {r // q for r in rows} == {0, 1, 2, 3}
    return (_engine(prf, D, e),) + \
        _keys_and_shares(prf, D, e, rows, WIDE_BINS)


def _batch_of(keys, batch):
    return torch.stack([keys[i % len(keys)] for i in range(batch)])


def _bins_of(bins, batch):
    return [bins[i % len(bins)] for i in range(batch)]


def _check(case, bins, e, batches):
    dpf, want, k1s, k2s, cpu1, cpu2 = case
    for batch in batches:
        idx = np.arange(batch) % len(bins)
        bb = _bins_of(bins, batch)
        a = dpf.eval_gpu(_batch_of(k1s, batch), bb).numpy()
        b = dpf.eval_gpu(_batch_of(k2s, batch),
                         torch.tensor(bb, dtype=torch.int64)).numpy()
        assert a.shape == (batch, e) and a.dtype == np.int32
        assert np.array_equal(a, cpu1[idx][:, :e]), batch
        assert np.array_equal(b, cpu2[idx][:, :e]), batch
        assert np.array_equal(so.reconstruct(a, cpu2[idx][:, :e]),
                              want[idx][:, :e]), batch
    assert dpf._plan is None       # eval_gpu binds nothing


# ---------------------------------------------------------------------------
# Lattice, 16 words
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", DEPTHS)
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_packed_binned_matches_cpu(prf, D, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    zlog = _core.zlog_for_depth(D)
    for batch, slog in zip(BATCHES, SLOG[D]):
        assert _hip.eval_slog(batch, D, zlog) == slog, (D, batch)
    _check(_case(prf, D), KEY_BINS, 16, BATCHES)


@pytest.mark.parametrize("D", DEPTHS)
def test_gpu_device_blocks_are_the_host_layout(D):
    dpf = _case(DPF.PRF_SALSA20, D)[0]
    for b in range(dpf.num_bins):
        assert torch.equal(dpf._table_gpu[b].cpu(), dpf.bin_block(b)), b


# ---------------------------------------------------------------------------
# Wide rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("e", [17, 32, 33, 64])
@pytest.mark.parametrize("D", [7, 11, 12])
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_packed_binned_wide_matches_cpu(prf, D, e, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    case = _wide_case(prf, D, e)
    assert case[0]._entry_padded == {17: 32, 32: 32, 33: 48, 64: 64}[e]
    assert case[0].fused_servable
    _check(case, WIDE_BINS, e, [1, 3, 5] + ([1025] if D == 7 else []))


# ---------------------------------------------------------------------------
# AES units per workgroup
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("e", [16, 64])
@pytest.mark.parametrize("D", [12, 16])
@pytest.mark.parametrize("units", [1, 2, 3, 4])
def test_gpu_packed_binned_aes_units(units, D, e, monkeypatch):
    """Every K the build has, forced; a forced K above the cap is clamped to
    it.  Batch 7: units of different bins share a workgroup."""
    monkeypatch.setenv("GPUDPF_AES_UNITS", str(units))
    prf = DPF.PRF_AES128
    cap = 3 if e == 16 else 2
    for n_units in (7, 768, 1000):
        assert _hip.eval_units_per_wg_packed(prf, n_units, e) \
            == min(units, cap)
    assert _hip.eval_units_per_wg(prf, 1000) == units    # plain: unchanged
    if e == 16:
        _check(_case(prf, D), KEY_BINS, 16, [7])
    else:
        _check(_wide_case(prf, D, e), WIDE_BINS, e, [7])


def test_gpu_packed_binned_aes_units_default(monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    for n_units in (1, 256, 2048):
        assert _hip.eval_units_per_wg_packed(DPF.PRF_AES128, n_units, 16) == 3
        for words in (32, 48, 64):
            assert _hip.eval_units_per_wg_packed(DPF.PRF_AES128, n_units,
                                                 words) == 2


# ---------------------------------------------------------------------------
# One bin is the packed engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 11])
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_one_bin_is_the_packed_engine(prf, D, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    n = (4 << D) - 5
    table = _rand((n, 16), 31 + D)
    packed = PackedDPF(prf=prf)
    packed.eval_init(table)
    binned = PackedBinnedDPF(prf=prf)
    binned.eval_init([table])
    assert torch.equal(binned._table_gpu[0], packed._table_gpu)
    for batch in (3, 65):
        keys, _ = packed.gen_batch([(i * 389 + 5) % n for i in range(batch)],
                                   n)
        want = packed.eval_gpu(keys)
        assert torch.equal(binned.eval_gpu(keys, [0] * batch), want)
    assert np.array_equal(
        want[0].numpy(),
        _core.eval_fused_cpu(keys[0].numpy(), _padded(table, 4 << D, 16), prf))


# ---------------------------------------------------------------------------
# Raw launches into buffers of exactly their size, carved from guard-filled
# tensors.  Keys of the last bin read rows that end where the table ends.
# ---------------------------------------------------------------------------
def _guarded(words, device):
    return torch.full((words + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32,
                      device=device)


def _guards_intact(big, words):
    return bool((big[:GUARD_WORDS] == GUARD).all().item()) and \
        bool((big[GUARD_WORDS + words:] == GUARD).all().item())


@pytest.mark.parametrize("e", [16, 64])
@pytest.mark.parametrize("D", [7, 16])
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_packed_binned_raw_launches_stay_in_bounds(prf, D, e, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    if e == 16:
        dpf, _w, k1s, _k2s, cpu1, _c2 = _case(prf, D)
        bins, batch = KEY_BINS, 7
    else:
        dpf, _w, k1s, _k2s, cpu1, _c2 = _wide_case(prf, D, e)
        bins, batch = WIDE_BINS, 5
    assert bins[0] == dpf.num_bins - 1     # key 0 reads the last block
    n, zlog = 4 << D, dpf._zlog
    dev = dpf._table_gpu.device
    assert dpf._table_gpu.numel() == dpf.num_bins * n * e
    stream = torch.cuda.current_stream(dev).cuda_stream
    keys_gpu = torch.stack(k1s).to(dev).contiguous()
    bins_gpu = torch.tensor(bins, dtype=torch.int32, device=dev)
    need = dpf._scratch_bytes(batch)
    slog = _hip.eval_slog(batch, D, zlog)
    assert need == _hip.eval_scratch_bytes(batch, D, zlog)
    assert need == (batch << slog) * max(0, D - zlog - 7) * (1 << zlog) * 16
    assert (need > 0) == (D == 16)
    sw = need // 4
    scratch = _guarded(sw, dev)
    sptr = scratch.data_ptr() + GUARD_WORDS * 4 if need else 0
    out = _guarded(batch * e, dev)
    out[GUARD_WORDS:GUARD_WORDS + batch * e] = 0
    optr = out.data_ptr() + GUARD_WORDS * 4
    _hip.eval_fused_packed_binned(
        keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(), bins_gpu.data_ptr(),
        optr, dpf._aes_ptr, batch, n, D, zlog, dpf.num_bins, prf, stream,
        sptr, need, e)
    torch.cuda.synchronize(dev)
    got = out[GUARD_WORDS:GUARD_WORDS + batch * e].view(batch, e).cpu()
    assert np.array_equal(got.numpy(), cpu1)
    assert _guards_intact(out, batch * e)
    assert _guards_intact(scratch, sw)

    # raised on the host, before any launch: one byte of scratch short, no
    # bins, no bin or too many, an unaligned out, the plain row count
    out = _guarded(batch * e, dev)
    optr = out.data_ptr() + GUARD_WORDS * 4
    good = dict(bins=bins_gpu.data_ptr(), out=optr, n=n,
                num_bins=dpf.num_bins, scratch=sptr, scratch_bytes=need)
    bad = [dict(bins=0), dict(num_bins=0), dict(num_bins=1 << 60),
           dict(out=optr + 4), dict(n=1 << D)]
    if need:
        bad.append(dict(scratch_bytes=need - 1))
    for change in bad:
        kw = dict(good)
        kw.update(change)
        with pytest.raises(ValueError):
            _hip.eval_fused_packed_binned(
                keys=keys_gpu.data_ptr(), table=dpf._table_gpu.data_ptr(),
                aes_tabs=dpf._aes_ptr, batch=batch, depth=D, zlog=zlog,
                prf=prf, stream=stream, entry_words=e, **kw)
    torch.cuda.synchronize(dev)
    assert bool((out == GUARD).all().item())


# ---------------------------------------------------------------------------
# Servers: unchanged GraphedServer / PipelinedServer over a bound slot plan
# ---------------------------------------------------------------------------
# the plan [4, 0, 2, 2, 4] by the fixture's keys, two ways
SLOT_KEYS = [[0, 1, 2, 3, 4], [4, 1, 3, 2, 0]]
PLAN = [4, 0, 2, 2, 4]


def _server_batches(prf):
    _dpf, _want, k1s, k2s, cpu1, cpu2 = _case(prf, 16)
    out = []
    for keys, cpu, order in [(k1s, cpu1, SLOT_KEYS[0]),
                             (k2s, cpu2, SLOT_KEYS[0]),
                             (k1s, cpu1, SLOT_KEYS[1])]:
        out.append((torch.stack([keys[i] for i in order]), cpu[order]))
    return out


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_SALSA20],
                         ids=PRF_IDS.get)
def test_gpu_servers_serve_packed_binned(prf, monkeypatch):
    from gpudpf.serving import GraphedServer, PipelinedServer

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    for order in SLOT_KEYS:
        assert [KEY_BINS[i] for i in order] == PLAN
    batches = _server_batches(prf)
    dpf = _engine(prf, 16)
    dev = dpf._table_gpu.device
    dev_plan = dpf.bind_bins(PLAN)
    assert dev_plan.device == dev and dev_plan.tolist() == PLAN
    assert dpf._scratch_bytes(5) > 0       # the slots own real scratch
    graphed = GraphedServer(dpf, batch=5)
    assert not graphed.wide
    for keys, cpu in batches:
        assert np.array_equal(graphed.eval(keys).numpy(), cpu)
    piped = PipelinedServer(dpf, batch=5, depth=2)
    h0 = piped.submit(batches[0][0])
    h1 = piped.submit(batches[1][0])       # two in flight before collecting
    assert np.array_equal(piped.collect(h0).numpy(), batches[0][1])
    h2 = piped.submit(batches[2][0])
    assert np.array_equal(piped.collect(h1).numpy(), batches[1][1])
    assert np.array_equal(piped.collect(h2).numpy(), batches[2][1])
    # eval_gpu_into, and an eval_gpu with other bins leaves the plan bound
    out = torch.full((5, 16), 7, dtype=torch.int32, device=dev)
    dpf.eval_gpu(batches[0][0][:2], [4, 0])
    assert dpf._plan is dev_plan
    dpf.eval_gpu_into(batches[2][0].to(dev), out)
    assert np.array_equal(out.cpu().numpy(), batches[2][1])


@pytest.mark.parametrize("queries_per_bin,group_size", [(1, 1), (2, 2)])
def test_gpu_serve_round_trip_packed(queries_per_bin, group_size):
    """pir.serve end to end, both servers' shares from the GPU: one through
    a GraphedServer, the other through a PipelinedServer."""
    from gpudpf.serving import GraphedServer, PipelinedServer
    from test_binned_cpu import plan, requests, round_trip

    opt, table, pats = plan(queries_per_bin, group_size)
    words = 64 if group_size == 2 else 16
    dpf = PackedBinnedDPF(prf=DPF.PRF_CHACHA20, fused_words=words)
    dpf.eval_init(serve.bin_tables(opt, table, max_words=words))
    bins = serve.slot_bins(opt)
    dpf.bind_bins(bins)
    graphed = GraphedServer(dpf, batch=len(bins))
    piped = PipelinedServer(dpf, batch=len(bins))
    turn = []

    def shares(keys):          # round_trip asks for server 1, then server 2
        turn.append(0)
        want = dpf.eval_cpu(keys, bins)
        if len(turn) % 2:
            got = graphed.eval(keys)
        else:
            got = piped.collect(piped.submit(keys))
        assert torch.equal(got, want)
        return got

    n_rec = sum(len(round_trip(opt, table, dpf, idx, shares))
                for idx in requests(opt, pats))
    assert n_rec > 0 and len(turn) == 2 * len(requests(opt, pats))


# ---------------------------------------------------------------------------
# Host errors: nothing is launched (the output keeps its guard pattern)
# ---------------------------------------------------------------------------
def test_gpu_packed_binned_host_errors_launch_nothing(monkeypatch):
    monkeypatch.delenv("GPUDPF_DEBUG", raising=False)
    prf, D = DPF.PRF_SALSA20, 9
    _d, _want, k1s, _k2s, cpu1, _c2 = _case(prf, D)
    dpf = _engine(prf, D)
    dev = dpf._table_gpu.device
    keys = torch.stack(k1s[:3])
    keys_gpu = keys.to(dev)
    out = torch.full((3, 16), GUARD, dtype=torch.int32, device=dev)

    with pytest.raises(Exception, match="bind_bins"):
        dpf._launch_fused(keys_gpu, out)
    for bad, msg in [([4, 5, 2], r"\[0, 5\)"), ([4, -1, 2], r"\[0, 5\)"),
                     ([4.0, 0.0, 2.0], "integers"),
                     (torch.tensor([[4, 0, 2]]), "1-D"),
                     (torch.tensor([4, 0, 2], device=dev), "on the host")]:
        with pytest.raises(Exception, match=msg):
            dpf.bind_bins(bad)
        with pytest.raises(Exception, match=msg):
            dpf.eval_gpu(keys, bad)
    assert dpf._plan is None
    with pytest.raises(Exception, match="bins: 2 ids for 3 keys"):
        dpf.eval_gpu(keys, [4, 0])
    dpf.bind_bins([4, 0])
    with pytest.raises(Exception, match="2 slots but the batch has 3"):
        dpf._launch_fused(keys_gpu, out)
    plan = dpf.bind_bins(KEY_BINS[:3])
    for bad in (plan.to(torch.int64), plan.cpu()):
        with pytest.raises(Exception, match="^bins must be"):
            dpf._launch_binned(keys_gpu, bad, out)
    with pytest.raises(Exception, match="^out must be"):
        dpf._launch_fused(keys_gpu, out[:, :15].contiguous())
    # plain keys of the same domain
    plain, _ = _core.gen(0, 4 << D, b"\x01" * 128, prf)
    with pytest.raises(Exception, match="packed keys"):
        dpf.eval_gpu([torch.from_numpy(plain)], [0])
    with pytest.raises(NotImplementedError):
        dpf.eval_gpu(keys, KEY_BINS[:3], one_hot_only=True)
    with pytest.raises(NotImplementedError):
        dpf.eval_gpu(keys, KEY_BINS[:3], strategy="two_stage")
    # a table wider than fused_words: refused at eval_init, by either width
    narrow = PackedBinnedDPF(prf=prf)
    with pytest.raises(Exception, match="at most 16"):
        narrow.eval_init([_rand((8, 17), 1)])
    mid = PackedBinnedDPF(prf=prf, fused_words=32)
    with pytest.raises(Exception, match="at most 32"):
        mid.eval_init([_rand((8, 33), 1)])
    torch.cuda.synchronize(dev)
    assert bool((out == GUARD).all().item())   # nothing was launched

    # and the correct launch after all of them is exact
    out.zero_()
    dpf._launch_fused(keys_gpu, out)
    assert np.array_equal(out.cpu().numpy(), cpu1[:3])


# ---------------------------------------------------------------------------
# The bin block offset past 2^32 elements
# ---------------------------------------------------------------------------
def _need(peak_gib):
    """Skip only when the device cannot hold the test's peak plus 4 GiB."""
    gc.collect()
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    if free < (peak_gib + 4) * GIB:
        pytest.skip("needs %d GiB of free device memory (peak %d GiB + 4), "
                    "%.1f GiB free" % (peak_gib + 4, peak_gib, free / GIB))


def test_gpu_packed_binned_block_offset_past_2_32_elements():
    """PEAK 20 GiB: 5 bins of n = 4 << 24 rows of 16 words.  Bin 4's block
    starts at element 2^32, bin 2's at element 2^31, bin 1's at byte 2^32.
    Every bin holds its own S (test_packed_binned_cpu.py proves where it
    lies), so a key that reads another bin's block, or a block offset that
    wrapped to bin 0, gives a different share."""
    _need(20)
    prf = DPF.PRF_DUMMY
    D, bins = pbo.LARGE_D, [4, 0, 2, 4, 1]
    n, zlog = pbo.LARGE_N, 8
    dev = torch.device("cuda:0")
    sts = pbo.large_bin_tables()
    table = torch.zeros((5 * n, 16), dtype=torch.int32, device=dev)
    assert table.numel() == 5 << 30
    for b, st in enumerate(sts):
        rows = torch.tensor([b * n + r for r in st.prow], dtype=torch.int64,
                            device=dev)
        table[rows] = torch.from_numpy(st.rows).to(dev)
        assert np.array_equal(table[rows].cpu().numpy(), st.rows)
    # key i selects a member of its own bin's S, the highest row first
    alphas = [sts[b].alphas(2)[i // 3] for i, b in enumerate(bins)]
    assert po.packed_perm(alphas[0], D, zlog) == n - 1   # last row, bin 4
    k1s, k2s = po.gen_keys(alphas, n, prf, seed=24)
    want1 = np.stack([sts[b].share(k, prf) for b, k in zip(bins, k1s)])
    want2 = np.stack([sts[b].share(k, prf) for b, k in zip(bins, k2s)])
    secret = np.stack([sts[b].row_of(a) for b, a in zip(bins, alphas)])
    assert np.array_equal(so.reconstruct(want1, want2), secret)
    # the shares tell the bins apart
    other = np.stack([sts[(b + 1) % 5].share(k, prf)
                      for b, k in zip(bins, k1s)])
    assert not (other == want1).all(axis=1).any()

    keys_gpu = torch.from_numpy(np.stack(k1s)).to(dev)
    bins_gpu = torch.tensor(bins, dtype=torch.int32, device=dev)
    out = torch.zeros((5, 16), dtype=torch.int32, device=dev)
    assert _hip.eval_slog(5, D, zlog) == 8
    _hip.eval_fused_packed_binned(
        keys_gpu.data_ptr(), table.data_ptr(), bins_gpu.data_ptr(),
        out.data_ptr(), 0, 5, n, D, zlog, 5, prf,
        torch.cuda.current_stream(dev).cuda_stream, 0, 0, 16)
    got = out.cpu().numpy()
    assert np.array_equal(got, want1)
    assert np.array_equal(so.reconstruct(got, want2), secret)
    del table, out
    gc.collect()
    torch.cuda.empty_cache()
