"""The binned fused kernel (gpudpf.BinnedDPF) on the GPU.

Geometry: depths 7, 9, 11 and 16 are the smallest that reach each code path
of the eval kernel — Z = 64 with DS 1; Z = 256 with DS 1; DS 3, the first
j-split; DS 8 with one sibling-stack level in global scratch and slog up to
6.  Every run holds 5 bins of unequal size and 7 distinct (key, bin) pairs
with bins [4, 0, 2, 2, 4, 1, 3], replicated i % 7 to batches 3, 65 and 1025,
so units of different bins share a workgroup (AES K > 1) and the segments
of one key sit in different workgroups.

All comparisons are exact: one server's GPU shares against
_core.eval_fused_cpu(key, that key's own bin table), plus reconstruction.
The bin tables are independently random, so a key evaluated against the
wrong bin cannot match; the fixture asserts on the CPU that each key's share
against its own bin differs from its share against bin 0.
"""

import functools

import numpy as np
import pytest
import torch

from gpudpf import BinnedDPF, DPF, _core
from pir import BatchPIROptimize, PIRConfig, serve

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

pytestmark = pytest.mark.gpu

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
DEPTHS = [7, 9, 11, 16]
BATCHES = [3, 65, 1025]
# eval_slog(batch, depth): the largest s <= min(DS - 2, 8) with
# batch << s <= 2048, DS = depth - min(8, depth - 1)
SLOG = {7: [0, 0, 0], 9: [0, 0, 0], 11: [1, 1, 0], 16: [6, 4, 0]}
KEY_BINS = [4, 0, 2, 2, 4, 1, 3]
N_KEYS = len(KEY_BINS)
GUARD = 0x5A5A5A5A
GUARD_WORDS = 4096


def _sizes(depth):
    n = 1 << depth
    # a one-row bin, two that need padding, two that fill the domain; the
    # last bin is full, so its rows end where the device table ends
    return [n, 1, n // 2 + 13, n - 3, n]


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _tables(depth):
    return tuple(_rand((nb, 16), 1000 * depth + b)
                 for b, nb in enumerate(_sizes(depth)))


def _padded(t, n):
    p = np.zeros((n, 16), dtype=np.int32)
    p[: t.shape[0]] = t.numpy()
    return p


def _engine(prf, depth):
    d = BinnedDPF(prf=prf)
    d.eval_init(list(_tables(depth)))
    assert d._depth == depth and d._n_domain == 1 << depth
    assert d._table_gpu.shape == (5, 1 << depth, 16)
    return d


@functools.lru_cache(maxsize=None)
def _case(prf, depth):
    """Per-(prf, depth) fixture, built once and never modified (eval_gpu
    leaves the engine as it is): engine, 7 key pairs, rows, CPU shares."""
    n = 1 << depth
    tabs = _tables(depth)
    sizes = _sizes(depth)
    rng = np.random.default_rng(prf * 100 + depth)
    rows = [n - 1, 0, int(rng.integers(1, sizes[2] - 1)), sizes[2] - 1,
            int(rng.integers(0, n - 1)), 0, int(rng.integers(0, sizes[3]))]
    k1s, k2s = [], []
    for r in rows:
        seed = bytes(rng.integers(0, 256, 128, dtype=np.uint8))
        k1, k2 = _core.gen(r, n, seed, prf)
        k1s.append(torch.from_numpy(k1))
        k2s.append(torch.from_numpy(k2))
    pad = [_padded(t, n) for t in tabs]
    cpu1 = np.stack([_core.eval_fused_cpu(k.numpy(), pad[b], prf)
                     for k, b in zip(k1s, KEY_BINS)])
    cpu2 = np.stack([_core.eval_fused_cpu(k.numpy(), pad[b], prf)
                     for k, b in zip(k2s, KEY_BINS)])
    # the oracle itself: it reconstructs, and it tells the bins apart
    rec = (cpu1.astype(np.int64) - cpu2.astype(np.int64)).astype(np.int32)
    want = np.stack([tabs[b][r].numpy() for r, b in zip(rows, KEY_BINS)])
    assert np.array_equal(rec, want)
    for i, b in enumerate(KEY_BINS):
        if b != 0:
            wrong = _core.eval_fused_cpu(k1s[i].numpy(), pad[0], prf)
            assert not np.array_equal(wrong, cpu1[i]), i
    return _engine(prf, depth), want, k1s, k2s, cpu1, cpu2


def _batch_of(keys, batch):
    return torch.stack([keys[i % N_KEYS] for i in range(batch)])


def _bins_of(batch):
    return [KEY_BINS[i % N_KEYS] for i in range(batch)]


def _check(prf, depth):
    dpf, want, k1s, k2s, cpu1, cpu2 = _case(prf, depth)
    zlog = _core.zlog_for_depth(depth)
    assert dpf._zlog == zlog == min(8, depth - 1)
    for batch, slog in zip(BATCHES, SLOG[depth]):
        assert _hip.eval_slog(batch, depth, zlog) == slog, (depth, batch)
        idx = np.arange(batch) % N_KEYS
        bins = _bins_of(batch)
        a = dpf.eval_gpu(_batch_of(k1s, batch), bins).numpy()
        b = dpf.eval_gpu(_batch_of(k2s, batch),
                         torch.tensor(bins, dtype=torch.int64)).numpy()
        assert np.array_equal(a, cpu1[idx]), (depth, batch)
        assert np.array_equal(b, cpu2[idx]), (depth, batch)
        rec = (a.astype(np.int64) - b.astype(np.int64)).astype(np.int32)
        assert np.array_equal(rec, want[idx]), (depth, batch)
    assert dpf._plan is None       # eval_gpu binds nothing


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("prf", PRFS[:3], ids=PRF_IDS.get)
def test_gpu_binned_matches_cpu(prf, depth):
    _check(prf, depth)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("units", [None, 1, 2, 3, 4])
def test_gpu_binned_aes_matches_cpu(units, depth, monkeypatch):
    if units is None:
        monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    else:
        monkeypatch.setenv("GPUDPF_AES_UNITS", str(units))
        assert _hip.eval_units_per_wg(DPF.PRF_AES128, 1000) == units
    _check(DPF.PRF_AES128, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_gpu_device_blocks_are_the_host_layout(depth):
    dpf = _case(DPF.PRF_SALSA20, depth)[0]
    for b in range(dpf.num_bins):
        assert torch.equal(dpf._table_gpu[b].cpu(), dpf.bin_block(b)), b


@pytest.mark.parametrize("depth", [11, 16])
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_one_bin_is_the_plain_engine(prf, depth, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    n = (1 << depth) - 5
    table = _rand((n, 16), 31 + depth)
    plain = DPF(prf=prf)
    plain.eval_init(table)
    binned = BinnedDPF(prf=prf)
    binned.eval_init([table])
    assert torch.equal(binned._table_gpu[0], plain._table_gpu)
    for batch in (3, 65):
        keys, _ = plain.gen_batch([(i * 389 + 5) % n for i in range(batch)], n)
        want = plain.eval_gpu(keys)
        assert torch.equal(binned.eval_gpu(keys, [0] * batch), want)
    assert np.array_equal(
        want[0].numpy(), _core.eval_fused_cpu(
            keys[0].numpy(), _padded(table, 1 << depth), prf))


# ---------------------------------------------------------------------------
# Caller-owned output and scratch carved from guard-filled tensors, as
# test_gpu_caller_owned_buffers_stay_in_bounds does for the plain kernel.
# Keys 0 and 4 read the last bin, whose rows end where the table ends.
# ---------------------------------------------------------------------------
def _guarded(words, device):
    return torch.full((words + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32,
                      device=device)


def _guards_intact(big, words):
    head = big[:GUARD_WORDS]
    tail = big[GUARD_WORDS + words:]
    return bool((head == GUARD).all().item()) and \
        bool((tail == GUARD).all().item())


@pytest.mark.parametrize("batch", [3, 65])
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_binned_caller_owned_buffers_stay_in_bounds(prf, batch,
                                                        monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    depth = 16
    dpf, _want, k1s, _k2s, cpu1, _c2 = _case(prf, depth)
    n, zlog = 1 << depth, dpf._zlog
    dev = dpf._table_gpu.device
    assert dpf._table_gpu.numel() == 5 * n * 16
    stream = torch.cuda.current_stream(dev).cuda_stream
    keys_gpu = _batch_of(k1s, batch).to(dev).contiguous()
    bins_gpu = torch.tensor(_bins_of(batch), dtype=torch.int32, device=dev)
    assert KEY_BINS[0] == dpf.num_bins - 1
    need = _hip.eval_scratch_bytes(batch, depth, zlog)
    slog = _hip.eval_slog(batch, depth, zlog)
    assert need == (batch << slog) * 1 * (1 << zlog) * 16 > 0
    assert need == dpf._scratch_bytes(batch)
    sw = need // 4
    scratch = _guarded(sw, dev)
    out = _guarded(batch * 16, dev)
    out[GUARD_WORDS:GUARD_WORDS + batch * 16] = 0
    sptr = scratch.data_ptr() + GUARD_WORDS * 4
    optr = out.data_ptr() + GUARD_WORDS * 4
    _hip.eval_fused_binned(keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(),
                           bins_gpu.data_ptr(), optr, dpf._aes_ptr, batch, n,
                           depth, zlog, dpf.num_bins, prf, stream, sptr, need)
    torch.cuda.synchronize(dev)
    got = out[GUARD_WORDS:GUARD_WORDS + batch * 16].view(batch, 16).cpu()
    assert np.array_equal(got.numpy(), cpu1[np.arange(batch) % N_KEYS])
    assert _guards_intact(scratch, sw)
    assert _guards_intact(out, batch * 16)

    # one byte of scratch short, no bins, no bin or too many: raised on the
    # host, before any launch
    out = _guarded(batch * 16, dev)
    optr = out.data_ptr() + GUARD_WORDS * 4
    for bins_ptr, num_bins, nbytes in [
            (bins_gpu.data_ptr(), dpf.num_bins, need - 1),
            (0, dpf.num_bins, need),
            (bins_gpu.data_ptr(), 0, need),
            (bins_gpu.data_ptr(), -1, need),
            (bins_gpu.data_ptr(), 1 << 42, need)]:
        with pytest.raises(ValueError):
            _hip.eval_fused_binned(
                keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(), bins_ptr,
                optr, dpf._aes_ptr, batch, n, depth, zlog, num_bins, prf,
                stream, sptr, nbytes)
    torch.cuda.synchronize(dev)
    assert bool((out == GUARD).all().item())


# ---------------------------------------------------------------------------
# Servers: unchanged GraphedServer / PipelinedServer over a bound slot plan
# ---------------------------------------------------------------------------
# slot plan of 5 bins x 2 queries is [0,0,1,1,2,2,3,3,4,4]; the fixture's keys
# by bin: 0 -> key 1; 1 -> key 5; 2 -> keys 2, 3; 3 -> key 6; 4 -> keys 0, 4
SLOT_KEYS = [[1, 1, 5, 5, 2, 3, 6, 6, 0, 4], [1, 1, 5, 5, 3, 2, 6, 6, 4, 0]]


def _server_batches(prf):
    _dpf, _want, k1s, k2s, cpu1, cpu2 = _case(prf, 16)
    out = []
    for keys, cpu, order in [(k1s, cpu1, SLOT_KEYS[0]),
                             (k2s, cpu2, SLOT_KEYS[0]),
                             (k1s, cpu1, SLOT_KEYS[1])]:
        out.append((torch.stack([keys[i] for i in order]), cpu[order]))
    return out


def _bound_engine(prf):
    opt = BatchPIROptimize(
        64, [[1, 2]], pir=PIRConfig(num_bins=5, queries_per_bin=2))
    plan = serve.slot_bins(opt)
    assert plan == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert [KEY_BINS[i] for i in SLOT_KEYS[0]] == plan
    assert [KEY_BINS[i] for i in SLOT_KEYS[1]] == plan
    dpf = _engine(prf, 16)
    dev_plan = dpf.bind_bins(plan)
    assert dev_plan.device == dpf._table_gpu.device
    assert dev_plan.dtype == torch.int32 and dev_plan.tolist() == plan
    return dpf


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_SALSA20],
                         ids=PRF_IDS.get)
def test_gpu_graphed_server_serves_binned(prf, monkeypatch):
    from gpudpf.serving import GraphedServer

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    srv = GraphedServer(_bound_engine(prf), batch=10)
    for keys, cpu in _server_batches(prf):
        assert np.array_equal(srv.eval(keys).numpy(), cpu)


@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_SALSA20],
                         ids=PRF_IDS.get)
def test_gpu_pipelined_server_serves_binned(prf, monkeypatch):
    from gpudpf.serving import PipelinedServer

    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    dpf = _bound_engine(prf)
    assert dpf._scratch_bytes(10) > 0      # the slots own real scratch
    srv = PipelinedServer(dpf, batch=10, depth=2)
    batches = _server_batches(prf)
    h0 = srv.submit(batches[0][0])
    h1 = srv.submit(batches[1][0])         # two in flight before collecting
    assert np.array_equal(srv.collect(h0).numpy(), batches[0][1])
    h2 = srv.submit(batches[2][0])
    assert np.array_equal(srv.collect(h1).numpy(), batches[1][1])
    assert np.array_equal(srv.collect(h2).numpy(), batches[2][1])
    # eval_gpu_into and an eval_gpu with other bins leave the plan bound
    dev = dpf._table_gpu.device
    out = torch.full((10, 16), 7, dtype=torch.int32, device=dev)
    dpf.eval_gpu(batches[0][0][:3], [0, 0, 1])
    dpf.eval_gpu_into(batches[2][0].to(dev), out)
    assert np.array_equal(out.cpu().numpy(), batches[2][1])


@pytest.mark.parametrize("queries_per_bin,group_size", [(1, 1), (2, 2)])
def test_gpu_serve_round_trip(queries_per_bin, group_size):
    """pir.serve end to end, both servers' shares from the GPU: one through
    a GraphedServer, the other through a PipelinedServer."""
    from gpudpf.serving import GraphedServer, PipelinedServer
    from test_binned_cpu import plan, requests, round_trip

    opt, table, pats = plan(queries_per_bin, group_size)
    dpf = BinnedDPF(prf=DPF.PRF_CHACHA20)
    dpf.eval_init(serve.bin_tables(opt, table))
    bins = serve.slot_bins(opt)
    dpf.bind_bins(bins)
    graphed = GraphedServer(dpf, batch=len(bins))
    piped = PipelinedServer(dpf, batch=len(bins))
    turn = []

    def shares(keys):          # round_trip asks for server 1, then server 2
        turn.append(0)
        if len(turn) % 2:
            return graphed.eval(keys)
        got = piped.collect(piped.submit(keys))
        assert torch.equal(got, dpf.eval_cpu(keys, bins))
        return got

    n_rec = sum(len(round_trip(opt, table, dpf, idx, shares))
                for idx in requests(opt, pats))
    assert n_rec > 0 and len(turn) == 2 * len(requests(opt, pats))


# ---------------------------------------------------------------------------
# Host errors: nothing is launched (the output keeps its guard pattern)
# ---------------------------------------------------------------------------
def test_gpu_host_errors_launch_nothing(monkeypatch):
    monkeypatch.delenv("GPUDPF_DEBUG", raising=False)
    prf, depth = DPF.PRF_SALSA20, 9
    _d, _want, k1s, _k2s, cpu1, _c2 = _case(prf, depth)
    dpf = _engine(prf, depth)
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
    with pytest.raises(Exception, match="2 slots but the batch has 3"):
        dpf._launch_fused(keys_gpu, out, torch.empty(
            0, dtype=torch.uint8, device=dev))
    # the plan's own launch arguments
    plan = dpf.bind_bins(KEY_BINS[:3])
    for bad in (plan.to(torch.int64), plan.cpu(),
                torch.cat([plan, plan])[::2]):
        with pytest.raises(Exception, match="^bins must be"):
            dpf._launch_binned(keys_gpu, bad, out)
    with pytest.raises(Exception, match="^keys must be"):
        dpf._launch_fused(keys_gpu.to(torch.int64), out)
    with pytest.raises(Exception, match="^out must be"):
        dpf._launch_fused(keys_gpu, out[:, :15].contiguous())
    with pytest.raises(NotImplementedError):
        dpf.eval_gpu(keys, KEY_BINS[:3], one_hot_only=True)
    with pytest.raises(NotImplementedError):
        dpf.eval_gpu(keys, KEY_BINS[:3], strategy="two_stage")
    wide = BinnedDPF(prf=prf)
    with pytest.raises(Exception, match="at most 16"):
        wide.eval_init([_rand((8, 17), 1)])
    torch.cuda.synchronize(dev)
    assert bool((out == GUARD).all().item())   # nothing was launched

    # and the correct launch after all of them is exact
    out.zero_()
    dpf._launch_fused(keys_gpu, out)
    assert np.array_equal(out.cpu().numpy(), cpu1[:3])
