"""The AES T-table image in LDS and the cipher that reads it.

Every row of the 64 KiB table holds 32 copies of te0[e] followed by 32
copies of te2[e] = ror16(te0[e]); lane l reads copy l % 32, and a te2 lookup
is the te0 address read at +128 (csrc/hip/prf_device.h).  Three layers, all
exact:

  * image:  the staged table, word for word, at every workgroup size the
    eval kernel runs (the staging loop strides by the workgroup size);
  * cipher: pair, single and low outputs of the device cipher against
    _core.prf over seeds that put every one of 64 byte values at every one
    of the 16 byte positions (each position takes its own path through the
    hand-written rounds 1 and 2), in a count that leaves the last wave
    partly filled;
  * fused:  shares against _core.eval_fused_cpu where the kernel changes
    path: Z = 64 (one wave per unit, lanes 32-63 share copies with lanes
    0-31), Z = 256, every K, global scratch with the deepest j-split, and
    one wide and one binned launch.
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

PRF = DPF.PRF_AES128
LDS_WORDS = 16384


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------
# image
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected_image():
    """word e*64 + h*32 + c = te0[e] (h = 0) or ror16(te0[e]) (h = 1), from
    the CPU core's te0 alone."""
    te0 = _core.aes_gpu_tables().view(np.uint32)[:256]
    te2 = (te0 >> np.uint32(16)) | (te0 << np.uint32(16))
    rows = np.concatenate([np.repeat(te0[:, None], 32, axis=1),
                           np.repeat(te2[:, None], 32, axis=1)], axis=1)
    img = rows.reshape(-1)
    assert img.shape == (LDS_WORDS,)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("threads", [256, 512, 768, 1024])
def test_gpu_aes_lds_image(threads):
    want = _expected_image()
    out = torch.full((LDS_WORDS,), 0x5A5A5A5A, dtype=torch.int32,
                     device="cuda:0")
    _hip.probe_aes_lds(_hip.ensure_aes_tables(0), out.data_ptr(), threads,
                       _stream())
    got = out.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (
        "threads=%d: %d words differ, first at word %d (entry %d, half %d, "
        "copy %d): got %#x want %#x" % (
            threads, bad.size, bad[0], bad[0] >> 6, (bad[0] >> 5) & 1,
            bad[0] & 31, got[bad[0]], want[bad[0]]))


def test_gpu_aes_lds_probe_rejects_bad_launch():
    out = torch.zeros(LDS_WORDS, dtype=torch.int32, device="cuda:0")
    tabs = _hip.ensure_aes_tables(0)
    for threads in (0, 32, 100, 1088):
        with pytest.raises(ValueError):
            _hip.probe_aes_lds(tabs, out.data_ptr(), threads, _stream())
    with pytest.raises(ValueError):
        _hip.probe_aes_lds(tabs, 0, 256, _stream())


# ---------------------------------------------------------------------------
# cipher
# ---------------------------------------------------------------------------
def _byte_values():
    """64 distinct byte values: both ends, and a stride that mixes both
    parities (round 1 of the second child reads table entry ^ 1)."""
    vals = [0x00, 0x01, 0xFE, 0xFF]
    i = 0
    while len(vals) < 64:
        v = (37 * i + 11) & 0xFF
        if v not in vals:
            vals.append(v)
        i += 1
    return vals


def _structured_seeds():
    """[1026, 16] bytes: byte p = x over a fixed background for p in 0..15
    and the 64 values x, then all-zero and all-one."""
    background = np.array([(0xA5 ^ (17 * p)) & 0xFF for p in range(16)],
                          dtype=np.uint8)
    seeds = []
    for p in range(16):
        for x in _byte_values():
            s = background.copy()
            s[p] = x
            seeds.append(s)
    seeds.append(np.zeros(16, dtype=np.uint8))
    seeds.append(np.full(16, 0xFF, dtype=np.uint8))
    out = np.stack(seeds)
    assert out.shape == (1026, 16) and out.shape[0] % 64 != 0
    return out


def test_gpu_aes_cipher_structured_seeds():
    seeds = _structured_seeds()
    count = seeds.shape[0]
    words = np.ascontiguousarray(seeds).view("<u4")  # [count, 4] LE limbs
    gs = torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
    bufs = [torch.empty((count, 4), dtype=torch.int32, device="cuda:0")
            for _ in range(4)]
    lows = [torch.empty(count, dtype=torch.int32, device="cuda:0")
            for _ in range(2)]
    _hip.probe_prf(gs.data_ptr(), _hip.ensure_aes_tables(0),
                   bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                   bufs[3].data_ptr(), lows[0].data_ptr(), lows[1].data_ptr(),
                   count, PRF, _stream())
    pair0, pair1, single0, single1 = (b.cpu().numpy().view(np.uint32)
                                      for b in bufs)
    low0, low1 = (l.cpu().numpy().view(np.uint32) for l in lows)
    want = np.empty((2, count, 4), dtype=np.uint32)
    for i in range(count):
        s_lo = int(words[i, 0]) | (int(words[i, 1]) << 32)
        s_hi = int(words[i, 2]) | (int(words[i, 3]) << 32)
        for pos in (0, 1):
            lo, hi = _core.prf(PRF, s_lo, s_hi, pos)
            v = (int(hi) << 64) | int(lo)
            want[pos, i] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(4)]
    for pos, pair, single, low in ((0, pair0, single0, low0),
                                   (1, pair1, single1, low1)):
        assert np.array_equal(pair, want[pos]), ("pair", pos)
        assert np.array_equal(single, want[pos]), ("single", pos)
        assert np.array_equal(low, want[pos][:, 0]), ("low", pos)


# ---------------------------------------------------------------------------
# fused
# ---------------------------------------------------------------------------
def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


def _keys(rows, n, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(
        _core.gen(r, n, bytes(rng.integers(0, 256, 128, dtype=np.uint8)),
                  PRF)[0]) for r in rows]


@functools.lru_cache(maxsize=None)
def _fused_case(depth, batch, words=16):
    """Engine with a resident table, `batch` keys of one server and their
    CPU shares; built once and never modified."""
    n = 1 << depth
    table = _rand((n, words), 7000 + depth + words)
    rng = np.random.default_rng(depth)
    rows = [0, n - 1] + [int(r) for r in rng.integers(1, n - 1, batch - 2)]
    keys = _keys(rows, n, 100 + depth)
    dpf = DPF(prf=PRF, fused_words=words)
    dpf.eval_init(table)
    cpu = np.stack([_core.eval_fused_cpu(k.numpy(), table.numpy(), PRF)
                    for k in keys])
    return dpf, keys, cpu


# depth -> (batch, Z, slog)
POINTS = {7: (5, 64, 0), 9: (5, 256, 0), 12: (5, 256, 2), 16: (3, 256, 6)}


def _check_fused(depth):
    batch, z, slog = POINTS[depth]
    dpf, keys, cpu = _fused_case(depth, batch)
    assert 1 << dpf._zlog == z
    assert _hip.eval_slog(batch, depth, dpf._zlog) == slog
    got = dpf.eval_gpu(keys).numpy()
    assert np.array_equal(got, cpu), depth


@pytest.mark.parametrize("depth", [7, 9, 16])
def test_gpu_aes_fused_matches_cpu(depth, monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    _check_fused(depth)


@pytest.mark.parametrize("units", [1, 2, 3, 4])
def test_gpu_aes_fused_every_k(units, monkeypatch):
    monkeypatch.setenv("GPUDPF_AES_UNITS", str(units))
    assert _hip.eval_units_per_wg(PRF, 5 << 2) == units
    _check_fused(12)


def test_gpu_aes_fused_wide_rows(monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    dpf, keys, cpu = _fused_case(8, 3, words=32)
    assert dpf.fused_servable
    got = dpf.eval_gpu(keys, strategy="fused").numpy()
    assert got.shape == (3, 32)
    assert np.array_equal(got, cpu)


def test_gpu_aes_fused_binned(monkeypatch):
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    depth, bins = 8, [2, 0, 1, 2, 1]
    n = 1 << depth
    tables = [_rand((n, 16), 9000 + b) for b in range(3)]
    keys = _keys([n - 1, 0, 77, 130, 255], n, 555)
    dpf = BinnedDPF(prf=PRF)
    dpf.eval_init(tables)
    cpu = np.stack([_core.eval_fused_cpu(k.numpy(), tables[b].numpy(), PRF)
                    for k, b in zip(keys, bins)])
    got = dpf.eval_gpu(torch.stack(keys), bins).numpy()
    assert np.array_equal(got, cpu)
