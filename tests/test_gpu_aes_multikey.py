"""AES fused kernel with several (key, segment) units per workgroup.

The AES eval kernel packs K units into one workgroup so they share the
64 KiB replicated T-table; K is chosen per launch and can be forced with
GPUDPF_AES_UNITS.  These tests force every K over batches that leave every
remainder mod K (surplus units in the last workgroup), at the domain sizes
where the kernel changes path: Z = 64/128/256 with DS = 1 (n = 128, 256,
512), the first LDS stack level (n = 2^12) and the first global-scratch
level (n = 2^16).  All comparisons are exact: GPU shares against the CPU
evaluation of the same keys, and reconstruction from both key halves.
"""

import functools

import numpy as np
import pytest
import torch

from gpudpf import DPF

pytestmark = pytest.mark.gpu

PRF = DPF.PRF_AES128
NS = [128, 256, 512, 1 << 12, 1 << 16]
BATCHES = [1, 2, 3, 5, 7, 9]
MAX_BATCH = max(BATCHES)
KMAX = 4


@functools.lru_cache(maxsize=None)
def _case(n):
    """Per-n fixture, computed once and never modified: engine with its
    table resident, MAX_BATCH key pairs, and the CPU shares of both halves."""
    g = torch.Generator().manual_seed(n)
    table = torch.randint(-(2**31), 2**31 - 1, (n, 16), dtype=torch.int64,
                          generator=g).to(torch.int32)
    # first, last and interior targets
    alphas = [0, n - 1] + [int(x) for x in
                           torch.randint(0, n, (MAX_BATCH - 2,), generator=g)]
    dpf = DPF(prf=PRF)
    k1s, k2s = [], []
    for a in alphas:
        k1, k2 = dpf.gen(a, n)
        k1s.append(k1)
        k2s.append(k2)
    dpf.eval_init(table)
    cpu1 = dpf.eval_cpu(k1s).numpy()
    cpu2 = dpf.eval_cpu(k2s).numpy()
    rec = (cpu1.astype(np.int64) - cpu2.astype(np.int64)).astype(np.int32)
    assert np.array_equal(rec, table[alphas].numpy())  # the oracle itself
    return dpf, table, alphas, k1s, k2s, cpu1, cpu2


def _check_all_batches(n):
    dpf, table, alphas, k1s, k2s, cpu1, cpu2 = _case(n)
    for batch in BATCHES:
        a = dpf.eval_gpu(k1s[:batch]).numpy()
        b = dpf.eval_gpu(k2s[:batch]).numpy()
        assert np.array_equal(a, cpu1[:batch]), (n, batch)
        assert np.array_equal(b, cpu2[:batch]), (n, batch)
        rec = (a.astype(np.int64) - b.astype(np.int64)).astype(np.int32)
        assert np.array_equal(rec, table[alphas[:batch]].numpy()), (n, batch)


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("n", NS)
def test_gpu_aes_multikey_fused_matches_cpu(n, k, monkeypatch):
    monkeypatch.setenv("GPUDPF_AES_UNITS", str(k))
    _check_all_batches(n)


@pytest.mark.parametrize("n", NS)
def test_gpu_aes_default_units_fused_matches_cpu(n, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _check_all_batches(n)


@pytest.mark.parametrize("k", [None, 3, 4])
def test_gpu_aes_multikey_onehot_matches_cpu(k, monkeypatch):
    n, batch = 1 << 12, 5
    if k is None:
        monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    else:
        monkeypatch.setenv("GPUDPF_AES_UNITS", str(k))
    dpf, _table, alphas, k1s, k2s, _c1, _c2 = _case(n)
    got1 = dpf.eval_gpu(k1s[:batch], one_hot_only=True).numpy()
    got2 = dpf.eval_gpu(k2s[:batch], one_hot_only=True).numpy()
    want1 = dpf.eval_cpu(k1s[:batch], one_hot_only=True).numpy()
    want2 = dpf.eval_cpu(k2s[:batch], one_hot_only=True).numpy()
    assert np.array_equal(got1, want1)
    assert np.array_equal(got2, want2)
    diff = (got1.astype(np.int64) - got2.astype(np.int64)).astype(np.int32)
    onehot = np.zeros((batch, n), dtype=np.int32)
    onehot[np.arange(batch), alphas[:batch]] = 1
    assert np.array_equal(diff[:, :n], onehot)


def test_gpu_aes_units_1_and_max_give_equal_shares(monkeypatch):
    n, batch = 1 << 16, 7
    dpf, _table, _alphas, k1s, _k2s, cpu1, _c2 = _case(n)
    monkeypatch.setenv("GPUDPF_AES_UNITS", "1")
    one = dpf.eval_gpu(k1s[:batch]).numpy()
    monkeypatch.setenv("GPUDPF_AES_UNITS", str(KMAX))
    many = dpf.eval_gpu(k1s[:batch]).numpy()
    assert np.array_equal(one, many)
    assert np.array_equal(one, cpu1[:batch])
