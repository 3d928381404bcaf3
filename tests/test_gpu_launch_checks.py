"""DPF._launch_*: the one checked path in front of every kernel launch.

Every clause of the argument checker raises before anything is launched,
a correct call after all the rejected ones is exact against the CPU core
(so the wrappers pass their arguments in the right order), caller-owned
scratch gives what the shared scratch gives, and the servers reject a
mistyped key batch instead of converting or broadcasting it into their
staging buffers.
"""

import functools

import numpy as np
import pytest
import torch

from gpudpf import DPF, _core

pytestmark = pytest.mark.gpu

PRF = DPF.PRF_SALSA20
N, BATCH = 1024, 3


def _table(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, (n, e), dtype=torch.int64,
                         generator=g).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(n=N, e=16, batch=BATCH):
    """(engine with the table resident, table, CPU keys, device keys);
    built once per shape and never modified."""
    dpf = DPF(prf=PRF)
    table = _table(n, e, 7)
    dpf.eval_init(table)
    keys, _ = dpf.gen_batch([(i * 389 + 5) % n for i in range(batch)], n)
    return dpf, table, keys, keys.to(dpf._table_gpu.device)


def _out(dpf, rows, cols, dtype=torch.int32):
    return torch.zeros((rows, cols), dtype=dtype, device=dpf._table_gpu.device)


# (id, argument the message must name, call) — one case per checker clause
REJECTED = [
    ("keys-int64", "keys", lambda d, k: d._launch_fused(
        k.to(torch.int64), _out(d, BATCH, 16))),
    ("keys-523", "keys", lambda d, k: d._launch_fused(
        k[:, :523].contiguous(), _out(d, BATCH, 16))),
    ("keys-strided", "keys", lambda d, k: d._launch_fused(
        torch.cat([k, k])[::2], _out(d, BATCH, 16))),
    ("keys-cpu", "keys", lambda d, k: d._launch_fused(
        k.cpu(), _out(d, BATCH, 16))),
    ("fused-out-15", "out", lambda d, k: d._launch_fused(
        k, _out(d, BATCH, 15))),
    ("fused-out-2rows", "out", lambda d, k: d._launch_fused(
        k, _out(d, BATCH - 1, 16))),
    ("out-int64", "out", lambda d, k: d._launch_fused(
        k, _out(d, BATCH, 16, torch.int64))),
    ("expand-out-short", "out", lambda d, k: d._launch_expand(
        k, _out(d, BATCH, N - 1))),
    ("scratch-float", "scratch", lambda d, k: d._launch_fused(
        k, _out(d, BATCH, 16), torch.zeros(
            64, dtype=torch.float32, device=k.device))),
]


@pytest.mark.parametrize("name,call", [(c[1], c[2]) for c in REJECTED],
                         ids=[c[0] for c in REJECTED])
def test_checker_rejects(name, call):
    dpf, _table_, _keys, keys_gpu = _case()
    with pytest.raises(Exception, match="^%s must be" % name):
        call(dpf, keys_gpu)


def test_uninitialised_dpf_rejected(monkeypatch):
    monkeypatch.delenv("GPUDPF_DEBUG", raising=False)
    _dpf, _table_, _keys, keys_gpu = _case()
    fresh = DPF(prf=PRF)
    out = torch.zeros((BATCH, 16), dtype=torch.int32, device=keys_gpu.device)
    with pytest.raises(Exception, match="eval_init"):
        fresh._launch_fused(keys_gpu, out)
    with pytest.raises(Exception, match="eval_init"):
        fresh.eval_gpu_into(keys_gpu, out)


def test_device_mismatch_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU to make the current device differ")
    dpf, _table_, _keys, keys_gpu = _case()
    with torch.cuda.device(1):
        with pytest.raises(Exception, match="current device"):
            dpf._launch_fused(keys_gpu, _out(dpf, BATCH, 16))


def test_correct_launches_exact_after_rejections():
    dpf, table, keys, keys_gpu = _case()
    for _id, name, call in REJECTED:
        with pytest.raises(Exception, match="^%s must be" % name):
            call(dpf, keys_gpu)
    out = _out(dpf, BATCH, 16)
    dpf._launch_fused(keys_gpu, out)
    shares = _out(dpf, BATCH, N)
    dpf._launch_expand(keys_gpu, shares)
    got = out.cpu().numpy()
    nat = shares.index_select(1, dpf._perm_gpu).cpu().numpy()
    for i in range(BATCH):
        k = keys[i].numpy()
        assert np.array_equal(
            got[i], _core.eval_fused_cpu(k, table.numpy(), PRF)), i
        assert np.array_equal(nat[i], _core.expand(k, PRF)), i


def test_caller_owned_scratch_matches_shared():
    # n = 2^16 is the smallest domain with a sibling-stack level in global
    # scratch; below it _scratch_bytes is 0 and nothing is exercised
    n = 1 << 16
    dpf, table, keys, keys_gpu = _case(n)
    need = dpf._scratch_bytes(BATCH)
    assert need > 0
    dev = keys_gpu.device

    shared = _out(dpf, BATCH, 16)
    dpf._launch_fused(keys_gpu, shared)
    own = _out(dpf, BATCH, 16)
    dpf._launch_fused(keys_gpu, own,
                      torch.empty(need, dtype=torch.uint8, device=dev))
    assert torch.equal(own, shared)
    got = shared.cpu().numpy()
    for i in range(BATCH):
        assert np.array_equal(got[i], _core.eval_fused_cpu(
            keys[i].numpy(), table.numpy(), PRF)), i

    shared = _out(dpf, BATCH, n)
    dpf._launch_expand(keys_gpu, shared)
    own = _out(dpf, BATCH, n)
    dpf._launch_expand(keys_gpu, own,
                       torch.empty(need, dtype=torch.uint8, device=dev))
    assert torch.equal(own, shared)

    # one byte short raises on the host (the launcher's own size check)
    short = torch.empty(need - 1, dtype=torch.uint8, device=dev)
    with pytest.raises(Exception, match="scratch"):
        dpf._launch_fused(keys_gpu, _out(dpf, BATCH, 16), short)
    with pytest.raises(Exception, match="scratch"):
        dpf._launch_expand(keys_gpu, _out(dpf, BATCH, n), short)


def _serve(kind, dpf, keys):
    from gpudpf import serving

    srv = getattr(serving, kind)(dpf, keys.shape[0])
    if kind == "GraphedServer":
        return srv, srv.eval
    return srv, lambda k: srv.collect(srv.submit(k))


@pytest.mark.parametrize("kind,e", [("GraphedServer", 16),
                                    ("PipelinedServer", 16),
                                    ("TwoStageServer", 24)])
def test_servers_reject_mistyped_batches(kind, e):
    dpf, _table_, keys, _keys_gpu = _case(N, e, 4)
    _srv, run = _serve(kind, dpf, keys)
    with pytest.raises(Exception, match="keys must be int32"):
        run(keys.to(torch.int64))
    with pytest.raises(Exception, match="keys must be int32"):
        run(keys[:, :523].contiguous())
    want = dpf.eval_gpu(keys)
    assert want.shape == (4, e)
    assert torch.equal(run(keys), want)
    assert torch.equal(run([k for k in keys]), want)
