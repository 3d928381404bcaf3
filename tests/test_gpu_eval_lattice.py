"""dpf_eval_kernel (fused and one-hot expand) over every launch geometry.

The kernel changes code path with two launch parameters:

  DS = depth - zlog   where each sibling-stack level lives: none (DS 1),
                      rtop1 / rtop2 registers (DS 2, 3), 1..4 LDS levels
                      (DS 4..7, the `shared` slice growing past the
                      ping-pong at DS 6), 1..5 global-scratch levels
                      (DS 8..12).
  slog (j-split)      eval_slog(batch, DS) = the largest s <= min(DS-2, 8)
                      with batch << s <= 1024: 0 from batch 1025, 1 from
                      513, 2 from 257, ... 7 from 9, 8 up to batch 4.  It
                      sets the targeted entry descent, the segment bounds,
                      the scratch row and how many atomics meet per output
                      word.

The lattice is every depth 7..20 with every slog that depth can reach,
66 points: one each for DS 1 and 2 (depths 7..10), then min(DS-2, 8) + 1
for DS 3..12 (2+3+4+5+6+7+8+9+9+9).  A point below the depth's cap uses
batch (1024 >> s) + 1, the largest odd batch with that slog; the cap uses
batch 3.  Odd batches leave every remainder modulo the AES units per
workgroup (K = 1..4), and each test asserts through _hip.eval_slog that it
hit the geometry it names.

Every comparison is exact: GPU shares of one server against the CPU core
for the same keys (reconstruction a - b alone cancels whatever both servers
get equally wrong), plus reconstruction of table[alpha] from a GPU share
and a CPU share.
"""

import functools

import numpy as np
import pytest
import torch

from gpudpf import DPF, _core

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

gpu = pytest.mark.gpu

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
DEPTHS = list(range(7, 21))
N_KEYS = 7                 # coprime to every K = 2, 3, 4
LATTICE_POINTS = 66
EXPAND_MAX_BYTES = 256 << 20   # one-hot outputs above this are left out
EXPAND_HOST_BYTES = 64 << 20   # above this, compare on the device
EXPAND_LEFT_OUT = 15
GUARD = 0x5A5A5A5A


def _slog_cap(depth):
    ds = depth - _core.zlog_for_depth(depth)
    return max(0, min(ds - 2, 8))


def _points(depth):
    """(slog, batch) for every slog `depth` can reach."""
    cap = _slog_cap(depth)
    return [(s, (1024 >> s) + 1 if s < cap else 3) for s in range(cap + 1)]


def _lattice():
    return [(d, s, b) for d in DEPTHS for s, b in _points(d)]


def _expand_bytes(depth, batch):
    return batch * (1 << depth) * 4


def test_lattice_enumerator_matches_launcher():
    """No GPU needed: eval_slog is host arithmetic."""
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    pts = _lattice()
    assert len(pts) == LATTICE_POINTS
    assert len(set((d, s) for d, s, _ in pts)) == LATTICE_POINTS
    for depth, s, batch in pts:
        zlog = _core.zlog_for_depth(depth)
        assert _hip.eval_slog(batch, depth, zlog) == s, (depth, s, batch)
    # the lattice is complete: no batch reaches a slog outside it
    for depth in DEPTHS:
        zlog = _core.zlog_for_depth(depth)
        seen = {_hip.eval_slog(b, depth, zlog) for b in range(1, 1100)}
        assert seen == {s for s, _ in _points(depth)}, depth
    # DS covers 1..12 and the one-hot outputs left out are the 15 largest
    assert {d - _core.zlog_for_depth(d) for d in DEPTHS} == set(range(1, 13))
    out = [(d, s) for d, s, b in pts if _expand_bytes(d, b) > EXPAND_MAX_BYTES]
    assert len(out) == EXPAND_LEFT_OUT
    assert sorted(out) == [(d, s) for d in range(16, 21) for s in range(d - 15)]


def test_eval_scratch_bytes_matches_stack_placement():
    """No GPU needed.  An independent statement of the scratch contract: of
    the DS - 1 sibling-stack levels two live in registers, up to four in
    LDS, and each of the rest takes one Z-wide row of 16-byte seeds per
    (key, segment) unit."""
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    for depth in range(7, 33):
        zlog = _core.zlog_for_depth(depth)
        ds, z = depth - zlog, 1 << zlog
        for batch in (1, 3, 65, 512, 1025, 4096):
            slog = _hip.eval_slog(batch, depth, zlog)
            want = (batch << slog) * max(0, ds - 3 - 4) * z * 16
            assert _hip.eval_scratch_bytes(batch, depth, zlog) == want, \
                (depth, batch)


@pytest.mark.parametrize("depth,n", [(7, 256), (0, 1)])
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_naive_rejects_mismatched_domain(prf, depth, n):
    """No GPU needed: the naive launcher checks depth against n, like its
    siblings, before any HIP call, so null pointers never reach a kernel."""
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    with pytest.raises(ValueError, match="bad depth/n"):
        _hip.eval_naive(keys=0, out=0, aes_tabs=0, batch=1, n=n, depth=depth,
                        prf=prf, stream=0)


@pytest.mark.parametrize("depth,zlog", [(7, 5), (7, 7), (20, 20), (20, 0),
                                        (20, -1), (32, 33)])
@pytest.mark.parametrize("fused", [True, False])
def test_coop_rejects_zlog_out_of_range(fused, depth, zlog):
    """No GPU needed: the cooperative launcher checks zlog like the eval
    launchers, before any HIP call (its in-kernel row permutation shifts by
    32 - zlog and 33 - (depth - zlog))."""
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    with pytest.raises(ValueError, match="zlog must be in"):
        _hip.eval_coop(keys=0, table=0, out=0, aes_tabs=0, n=1 << depth,
                       depth=depth, zlog=zlog, prf=DPF.PRF_DUMMY, fused=fused,
                       stream=0)


@functools.lru_cache(maxsize=None)
def _table(depth):
    n = 1 << depth
    g = torch.Generator().manual_seed(1000 + depth)
    return torch.randint(-(2**31), 2**31, (n, 16), dtype=torch.int64,
                         generator=g).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(prf, depth):
    """Per-(prf, depth) fixture, built once and never modified: engine with
    the table resident, N_KEYS key pairs and the CPU shares of both halves."""
    n = 1 << depth
    table = _table(depth)
    tnp = table.numpy()
    rng = np.random.default_rng(prf * 100 + depth)
    alphas = [0, n - 1] + [int(x) for x in rng.integers(1, n - 1, N_KEYS - 2)]
    k1s, k2s = [], []
    for i, a in enumerate(alphas):
        seed = bytes(rng.integers(0, 256, 128, dtype=np.uint8))
        k1, k2 = _core.gen(a, n, seed, prf)
        k1s.append(torch.from_numpy(k1))
        k2s.append(torch.from_numpy(k2))
    assert len({k.numpy().tobytes() for k in k1s + k2s}) == 2 * N_KEYS
    cpu1 = np.stack([_core.eval_fused_cpu(k.numpy(), tnp, prf) for k in k1s])
    cpu2 = np.stack([_core.eval_fused_cpu(k.numpy(), tnp, prf) for k in k2s])
    rec = (cpu1.astype(np.int64) - cpu2.astype(np.int64)).astype(np.int32)
    assert np.array_equal(rec, tnp[alphas])  # the oracle itself
    dpf = DPF(prf=prf)
    dpf.eval_init(table)
    return dpf, tnp, alphas, k1s, k2s, cpu1, cpu2


def _batch_of(keys, batch):
    return torch.stack([keys[i % N_KEYS] for i in range(batch)])


def _check_fused(prf, depth):
    dpf, tnp, alphas, k1s, k2s, cpu1, cpu2 = _case(prf, depth)
    zlog = _core.zlog_for_depth(depth)
    for s, batch in _points(depth):
        assert _hip.eval_slog(batch, depth, zlog) == s, (depth, s, batch)
        idx = np.arange(batch) % N_KEYS
        a = dpf.eval_gpu(_batch_of(k1s, batch)).numpy()
        b = dpf.eval_gpu(_batch_of(k2s, batch)).numpy()
        assert np.array_equal(a, cpu1[idx]), (depth, s, batch)
        assert np.array_equal(b, cpu2[idx]), (depth, s, batch)
        rec = (a.astype(np.int64) - cpu2[idx].astype(np.int64)).astype(np.int32)
        assert np.array_equal(rec, tnp[np.asarray(alphas)[idx]]), (depth, s)


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("prf", PRFS[:3], ids=PRF_IDS.get)
def test_gpu_lattice_fused_matches_cpu(prf, depth):
    _check_fused(prf, depth)


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("units", [None, 1, 2, 3, 4])
def test_gpu_lattice_fused_aes_matches_cpu(units, depth, monkeypatch):
    if units is None:
        monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    else:
        monkeypatch.setenv("GPUDPF_AES_UNITS", str(units))
        assert _hip.eval_units_per_wg(DPF.PRF_AES128, 1000) == units
    _check_fused(DPF.PRF_AES128, depth)


@gpu
def test_gpu_lattice_auto_units_vary(monkeypatch):
    """The unforced AES runs above really take more than one K, and leave
    surplus units in the last workgroup."""
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    ks, surplus = set(), 0
    for _depth, s, batch in _lattice():
        n_units = batch << s
        k = _hip.eval_units_per_wg(DPF.PRF_AES128, n_units)
        assert 1 <= k <= 4
        ks.add(k)
        surplus += n_units % k != 0
        assert _hip.eval_units_per_wg(DPF.PRF_SALSA20, n_units) == 1
    assert len(ks) > 1, ks
    assert surplus > 0


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_gpu_lattice_expand_matches_cpu(prf, depth, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    dpf, _tnp, _alphas, k1s, k2s, _c1, _c2 = _case(prf, depth)
    zlog = _core.zlog_for_depth(depth)
    pts = [(s, b) for s, b in _points(depth)
           if _expand_bytes(depth, b) <= EXPAND_MAX_BYTES]
    assert len(_points(depth)) - len(pts) == max(0, depth - 15)
    for keys in (k1s, k2s):
        want = np.stack([_core.expand(k.numpy(), prf) for k in keys])
        want_dev = None
        for s, batch in pts:
            assert _hip.eval_slog(batch, depth, zlog) == s, (depth, s, batch)
            idx = np.arange(batch) % N_KEYS
            if _expand_bytes(depth, batch) <= EXPAND_HOST_BYTES:
                got = dpf.eval_gpu(_batch_of(keys, batch),
                                   one_hot_only=True).numpy()
                assert np.array_equal(got, want[idx]), (depth, s, batch)
                continue
            if want_dev is None:
                want_dev = torch.from_numpy(want).to(dpf._table_gpu.device)
            got = dpf.eval_gpu(_batch_of(keys, batch), one_hot_only=True,
                               out_device=True)
            full, rem = divmod(batch, N_KEYS)
            same = bool((got[:full * N_KEYS].view(full, N_KEYS, -1)
                         == want_dev).all().item())
            same = same and torch.equal(got[full * N_KEYS:], want_dev[:rem])
            del got
            assert same, (depth, s, batch)


# ---------------------------------------------------------------------------
# Caller-owned buffers: scratch of exactly eval_scratch_bytes and an output
# of exactly batch rows, both carved from the middle of larger tensors whose
# head and tail hold a pattern.  A sizing or indexing bug lands in memory
# the test owns and shows as a changed guard word.
# ---------------------------------------------------------------------------
GUARD_WORDS = 4096  # 16 KiB each side; keeps the carved scratch 16-B aligned


def _guarded(words, device):
    """int32 tensor [GUARD_WORDS | words | GUARD_WORDS] filled with GUARD."""
    return torch.full((words + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32,
                      device=device)


def _guards_intact(big, words):
    head = big[:GUARD_WORDS]
    tail = big[GUARD_WORDS + words:]
    return bool((head == GUARD).all().item()) and \
        bool((tail == GUARD).all().item())


@gpu
@pytest.mark.parametrize("batch", [3, 65])
@pytest.mark.parametrize("depth", [16, 18])
@pytest.mark.parametrize("prf", [DPF.PRF_AES128, DPF.PRF_CHACHA20],
                         ids=PRF_IDS.get)
def test_gpu_caller_owned_buffers_stay_in_bounds(prf, depth, batch,
                                                 monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    dpf, _tnp, _alphas, k1s, _k2s, cpu1, _c2 = _case(prf, depth)
    n = 1 << depth
    zlog = dpf._zlog
    dev = dpf._table_gpu.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    keys = _batch_of(k1s, batch)
    keys_gpu = keys.to(dev).contiguous()
    need = _hip.eval_scratch_bytes(batch, depth, zlog)
    slog = _hip.eval_slog(batch, depth, zlog)
    glob_levels = depth - zlog - 7
    assert glob_levels >= 1
    assert need == (batch << slog) * glob_levels * (1 << zlog) * 16
    sw = need // 4

    # fused: shared-scratch path first, then caller-owned buffers
    shared = dpf.eval_gpu(keys).numpy()
    assert np.array_equal(shared, cpu1[np.arange(batch) % N_KEYS])
    scratch = _guarded(sw, dev)
    out = _guarded(batch * 16, dev)
    out[GUARD_WORDS:GUARD_WORDS + batch * 16] = 0
    sptr = scratch.data_ptr() + GUARD_WORDS * 4
    optr = out.data_ptr() + GUARD_WORDS * 4
    _hip.eval_fused(keys_gpu.data_ptr(), dpf._table_gpu.data_ptr(), optr,
                    dpf._aes_ptr, batch, n, depth, zlog, prf, stream,
                    sptr, need)
    torch.cuda.synchronize(dev)
    got = out[GUARD_WORDS:GUARD_WORDS + batch * 16].view(batch, 16).cpu()
    assert np.array_equal(got.numpy(), shared)
    assert _guards_intact(scratch, sw)
    assert _guards_intact(out, batch * 16)

    # expand: rows in kernel order; compare with the shared-scratch launch
    ref = torch.empty((batch, n), dtype=torch.int32, device=dev)
    _hip.eval_expand(keys_gpu.data_ptr(), ref.data_ptr(), dpf._aes_ptr,
                     batch, n, depth, zlog, prf, stream)
    scratch = _guarded(sw, dev)
    out = _guarded(batch * n, dev)
    sptr = scratch.data_ptr() + GUARD_WORDS * 4
    optr = out.data_ptr() + GUARD_WORDS * 4
    _hip.eval_expand(keys_gpu.data_ptr(), optr, dpf._aes_ptr, batch, n,
                     depth, zlog, prf, stream, sptr, need)
    torch.cuda.synchronize(dev)
    assert torch.equal(out[GUARD_WORDS:GUARD_WORDS + batch * n].view(batch, n),
                       ref)
    assert _guards_intact(scratch, sw)
    assert _guards_intact(out, batch * n)
    # and the shared-scratch expand is the CPU expansion of key 0
    nat = ref[0].index_select(0, dpf._perm_gpu).cpu().numpy()
    assert np.array_equal(nat, _core.expand(k1s[0].numpy(), prf))

    # one byte short raises on the host, before any launch
    out = _guarded(batch * 16, dev)
    for launch in ("fused", "expand"):
        with pytest.raises(ValueError):
            if launch == "fused":
                _hip.eval_fused(keys_gpu.data_ptr(),
                                dpf._table_gpu.data_ptr(),
                                out.data_ptr() + GUARD_WORDS * 4,
                                dpf._aes_ptr, batch, n, depth, zlog, prf,
                                stream, sptr, need - 1)
            else:
                _hip.eval_expand(keys_gpu.data_ptr(), ref.data_ptr(),
                                 dpf._aes_ptr, batch, n, depth, zlog, prf,
                                 stream, sptr, need - 1)
    torch.cuda.synchronize(dev)
    assert bool((out == GUARD).all().item())  # nothing was launched
