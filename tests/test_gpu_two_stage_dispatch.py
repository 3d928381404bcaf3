"""The MFMA branch of DPF._eval_gpu_two_stage, end to end.

Wide entries (more than 16 words) go through expand + GEMM, and a chunk of
at least 128 keys on a table of at most 2 GiB takes ops.pir_matmul_u32
(digit planes + i8 MFMA); every smaller chunk takes the streaming GEMM.
Counting spies assert which GEMM each chunk took.  Each server's shares are
compared on their own with expand(key) @ table mod 2^32 from the CPU core
and numpy int64 (a - b alone cancels whatever both servers get equally
wrong), then table[alpha] is reconstructed.
"""

import numpy as np
import pytest
import torch

from gpudpf import DPF, _core, ops

pytestmark = pytest.mark.gpu

SEED = bytes(range(128))


def _table(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, (n, e), dtype=torch.int64,
                         generator=g).to(torch.int32)


def _alphas(n, batch):
    """Distinct-ish indices over the whole table, 0 and n - 1 included."""
    al = [(i * 389 + 5) % n for i in range(batch)]
    al[0], al[-1] = 0, n - 1
    return al


def _want_shares(keys, prf, table):
    """[batch, e] int32: expand(k) @ table mod 2^32, natural row order."""
    n = table.shape[0]
    t64 = table.numpy().astype(np.int64)
    hot = np.stack([_core.expand(k, prf)[:n] for k in keys]).astype(np.int64)
    return (hot @ t64).astype(np.uint32).astype(np.int32)


def _spy(monkeypatch):
    calls = {"mfma": [], "stream": []}
    real_mfma, real_stream = ops.pir_matmul_u32, ops.pir_matmul_u32_stream

    def mfma(shares, table):
        calls["mfma"].append(int(shares.shape[0]))
        return real_mfma(shares, table)

    def stream(shares, table, out=None):
        calls["stream"].append(int(shares.shape[0]))
        return real_stream(shares, table, out)

    monkeypatch.setattr(ops, "pir_matmul_u32", mfma)
    monkeypatch.setattr(ops, "pir_matmul_u32_stream", stream)
    return calls


CASES = [
    # n, entry width, prf, batch, MFMA chunks, streaming chunks
    (1024, 40, DPF.PRF_CHACHA20, 133, [128], [5]),
    (1024, 40, DPF.PRF_AES128, 133, [128], [5]),
    (1024, 17, DPF.PRF_CHACHA20, 133, [128], [5]),   # one over the fused limit
    (1024, 48, DPF.PRF_CHACHA20, 133, [128], [5]),   # no entry padding
    (5000, 40, DPF.PRF_CHACHA20, 128, [128], []),    # domain padded to 8192
]


@pytest.mark.parametrize(
    "n,e,prf,batch,mfma,stream", CASES,
    ids=["n%d-e%d-%s-b%d" % (c[0], c[1], DPF._PRF_NAMES[c[2]].lower(), c[3])
         for c in CASES])
def test_two_stage_takes_mfma_and_is_exact(monkeypatch, n, e, prf, batch,
                                           mfma, stream):
    dpf = DPF(prf=prf)
    table = _table(n, e, 40 + e)
    dpf.eval_init(table)
    alphas = _alphas(n, batch)
    k1s, k2s = _core.gen_batch(np.asarray(alphas, dtype=np.int64),
                               DPF._domain(n), SEED, prf)
    calls = _spy(monkeypatch)
    got = []
    for ks in (k1s, k2s):
        calls["mfma"].clear()
        calls["stream"].clear()
        got.append(dpf.eval_gpu(torch.from_numpy(ks)).numpy())
        assert calls["mfma"] == mfma
        assert calls["stream"] == stream
    for server, ks in enumerate((k1s, k2s)):
        want = _want_shares(ks, prf, table)
        assert got[server].shape == (batch, e)
        bad = np.argwhere(got[server] != want)
        assert len(bad) == 0, (server, "%d of %d words differ, first at %s"
                               % (len(bad), want.size, bad[0]))
    rec = (got[0].astype(np.int64) - got[1].astype(np.int64)).astype(np.int32)
    assert np.array_equal(rec, table.numpy()[alphas])
