"""MFMA mod-2^32 GEMM tests: exactness vs a wrapping int64 numpy
reference, including an accumulator-overflow case that proves i32 MFMA
accumulation wraps (not saturates); the launcher's K-split as host
arithmetic and on the GPU at the K where the slices once stopped short of
K; padding and tile edges; operands that drive the signed-digit borrow
chain; a fragment-layout probe; and the digit-plane kernel on its own,
up to the size at which its grid-stride loop runs."""

import time

import numpy as np
import pytest
import torch

from gpudpf import ops

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

gpu = pytest.mark.gpu

# (M, N, K) -> ksplit.  With kchunk = ceil(floor(K/ks)/64)*64 these left
# the last 64 or 192 rows of K unread.
SPLIT_SHORT = {(64, 16, 8256): 128, (64, 16, 16448): 256,
               (64, 16, 16576): 256, (128, 16, 16448): 256}
# Correct under either formula; (64, 16, 192) has an uneven last slice.
SPLIT_CONTROL = {(64, 16, 8192): 128, (64, 16, 8320): 128, (64, 16, 192): 2}
# M, N and K one below, at and one above a tile edge, several workgroups
# in x and y, rows in all four waves; the last pads up to a SPLIT_SHORT K.
PAD_SHAPES = [(1, 1, 1), (63, 15, 63), (65, 17, 65), (64, 16, 64),
              (130, 33, 129), (1, 1, 8256)]
# bytes 0x7F/0x80/0xFF at every position: the borrow of the signed
# base-256 decomposition starts, stops and runs through all four digits
EXTREME = np.array([0, 1, 0x7F, 0x80, 0xFF, 0x7F7F7F7F, 0x80808080,
                    0xFFFFFF80, 0x0000FF80, 0x7FFFFFFF, 0x80000000,
                    0xFFFFFFFF], dtype=np.uint32)


def _ref_mod32(a, b):
    # numpy int64 matmul wraps mod 2^64; truncating to uint32 is exact mod 2^32
    prod = a.astype(np.int64) @ b.astype(np.int64)
    return prod.astype(np.uint32).astype(np.int32)


def _random(rng, shape):
    return rng.integers(-(2**31), 2**31, shape, dtype=np.int64).astype(
        np.int32)


def _extreme(rng, shape):
    return rng.choice(EXTREME, size=shape).astype(np.int32)


def _padded(M, N, K):
    return -(-M // 64) * 64, -(-N // 16) * 16, -(-K // 64) * 64


def _check_matmul(a, b, tag):
    got = ops.pir_matmul_u32(torch.from_numpy(a), torch.from_numpy(b)).cpu()
    want = _ref_mod32(a, b)
    bad = np.argwhere(got.numpy() != want)
    assert len(bad) == 0, (tag, "%d of %d words differ, first at %s"
                           % (len(bad), want.size, bad[0]))


# ----------------------------------------------------------------------
# host arithmetic (no GPU)
# ----------------------------------------------------------------------
def test_gemm_u32_split_covers_k():
    """No GPU needed: gemm_u32_split is the launcher's own arithmetic."""
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    short = []
    for M in range(64, 8 * 64 + 1, 64):
        for N in range(16, 4 * 16 + 1, 16):
            for K in range(64, 2100 * 64 + 1, 64):
                ksplit, kchunk = _hip.gemm_u32_split(M, N, K)
                assert kchunk % 64 == 0, (M, N, K, ksplit, kchunk)
                assert ksplit >= 1, (M, N, K, ksplit, kchunk)
                assert ksplit & (ksplit - 1) == 0, (M, N, K, ksplit, kchunk)
                assert ksplit <= K // 64, (M, N, K, ksplit, kchunk)
                if ksplit * kchunk < K:
                    short.append((M, N, K, ksplit, kchunk))
    assert not short, "%d shapes leave K uncovered, e.g. %s" % (
        len(short), short[:4])
    for (M, N, K), want in {**SPLIT_SHORT, **SPLIT_CONTROL}.items():
        ksplit, kchunk = _hip.gemm_u32_split(M, N, K)
        assert ksplit == want, (M, N, K, ksplit)
        assert kchunk % 64 == 0 and ksplit * kchunk >= K, (
            M, N, K, ksplit, kchunk)


@pytest.mark.parametrize("M,N,K", [(63, 16, 64), (64, 15, 64), (64, 16, 65)])
def test_gemm_u32_mfma_rejects_unpadded(M, N, K):
    """No GPU needed: the shape check runs before anything is launched."""
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    with pytest.raises(ValueError):
        _hip.gemm_u32_mfma(0, 0, 0, M, N, K, 0)
    with pytest.raises(ValueError):
        _hip.gemm_u32_split(M, N, K)


# ----------------------------------------------------------------------
# the GEMM on the GPU
# ----------------------------------------------------------------------
@gpu
def test_gemm_u32_exact_random():
    rng = np.random.default_rng(11)
    for (M, N, K) in [(64, 16, 64), (128, 16, 4096), (100, 10, 1000),
                      (512, 16, 65536)]:
        a = rng.integers(-(2**31), 2**31 - 1, (M, K), dtype=np.int64).astype(
            np.int32
        )
        b = rng.integers(-(2**31), 2**31 - 1, (K, N), dtype=np.int64).astype(
            np.int32
        )
        got = ops.pir_matmul_u32(torch.from_numpy(a), torch.from_numpy(b)).cpu()
        want = torch.from_numpy(_ref_mod32(a, b))
        assert torch.equal(got, want), (M, N, K)


@gpu
def test_gemm_u32_accumulator_wraps():
    # worst-case digit magnitudes with K deep enough that the per-pair i32
    # MFMA accumulator exceeds 2^31: 128*128*2^18 = 2^32
    M, N, K = 64, 16, 1 << 18
    a = np.full((M, K), 0x80808080, dtype=np.uint32).astype(np.int32)
    b = np.full((K, N), 0x80808080, dtype=np.uint32).astype(np.int32)
    got = ops.pir_matmul_u32(torch.from_numpy(a), torch.from_numpy(b)).cpu()
    want = torch.from_numpy(_ref_mod32(a, b))
    assert torch.equal(got, want)


@gpu
def test_gemm_u32_one_hot_pir_identity():
    # one-hot share rows select table rows exactly
    M, N, K = 64, 16, 8192
    rng = np.random.default_rng(5)
    b = rng.integers(-(2**31), 2**31 - 1, (K, N), dtype=np.int64).astype(np.int32)
    a = np.zeros((M, K), dtype=np.int32)
    picks = rng.integers(0, K, M)
    a[np.arange(M), picks] = 1
    got = ops.pir_matmul_u32(torch.from_numpy(a), torch.from_numpy(b)).cpu()
    assert np.array_equal(got.numpy(), b[picks])


@gpu
@pytest.mark.parametrize(
    "M,N,K,ksplit",
    [k + (v,) for k, v in {**SPLIT_SHORT, **SPLIT_CONTROL}.items()],
    ids=lambda v: str(v))
def test_gemm_u32_k_split(M, N, K, ksplit):
    """Every K-slice is read: random operands, so a missing tail of K
    changes every output word."""
    assert _hip.gemm_u32_split(M, N, K)[0] == ksplit
    rng = np.random.default_rng(K + M)
    _check_matmul(_random(rng, (M, K)), _random(rng, (K, N)), (M, N, K))


@gpu
@pytest.mark.parametrize("M,N,K", PAD_SHAPES, ids=lambda v: str(v))
def test_gemm_u32_padding_and_tiles(M, N, K):
    rng = np.random.default_rng(1000 * M + K)
    if (M, N, K) == (1, 1, 8256):
        assert _hip.gemm_u32_split(*_padded(M, N, K))[0] == 128
    _check_matmul(_random(rng, (M, K)), _random(rng, (K, N)), (M, N, K))


@gpu
@pytest.mark.parametrize("M,N,K", PAD_SHAPES + [(64, 16, 8256)],
                         ids=lambda v: str(v))
def test_gemm_u32_extreme_operands(M, N, K):
    rng = np.random.default_rng(2000 * M + K)
    _check_matmul(_extreme(rng, (M, K)), _extreme(rng, (K, N)), (M, N, K))


@gpu
def test_gemm_u32_fragment_layout():
    """Row i of A selects k_i = (37 i + 5) % 128 — all different, over both
    64-blocks and all four k-groups — and B[k, j] = 16 k + j + 1 names its
    own position, so a wrong lane-to-(row, k) or (k, col) mapping gives a
    permuted or shifted row of B, not noise."""
    M, N, K = 64, 16, 128
    ks = (37 * np.arange(M) + 5) % K
    assert len(set(ks)) == M
    assert {k // 64 for k in ks} == {0, 1}
    assert {(k % 64) // 16 for k in ks} == {0, 1, 2, 3}
    a = np.zeros((M, K), dtype=np.int32)
    a[np.arange(M), ks] = 1
    b = (np.arange(K)[:, None] * 16 + np.arange(N)[None, :] + 1).astype(
        np.int32)
    got = ops.pir_matmul_u32(torch.from_numpy(a), torch.from_numpy(b)).cpu()
    for i in range(M):
        assert np.array_equal(got[i].numpy(), b[ks[i]]), (
            i, ks[i], got[i].tolist())


# ----------------------------------------------------------------------
# the digit-plane kernel on its own
# ----------------------------------------------------------------------
def _ref_digits(words):
    """[count] u32 -> [4, count] int64 signed base-256 digits, built by
    repeated division (the kernel carries a borrow byte by byte)."""
    v = words.astype(np.uint32).astype(np.int64)
    planes = []
    for _ in range(4):
        d = ((v + 128) & 0xFF) - 128
        planes.append(d)
        v = (v - d) >> 8
    return np.stack(planes)


def _check_digits(words_i32):
    got = ops._digit_planes(torch.from_numpy(words_i32).cuda()).cpu().numpy()
    assert got.dtype == np.int8 and got.shape == (4, words_i32.size)
    want = _ref_digits(words_i32)
    assert want.min() >= -128 and want.max() <= 127
    assert np.array_equal(got.astype(np.int64), want)
    total = sum(got[p].astype(np.int64) << (8 * p) for p in range(4))
    assert np.array_equal(total & 0xFFFFFFFF,
                          words_i32.astype(np.uint32).astype(np.int64))


@gpu
def test_digit_planes_edge_bytes():
    """Every pairing of 16-bit halves whose bytes are all digit-boundary
    values: the 49 halves with both bytes in the set, 2401 words."""
    edge = [0x00, 0x01, 0x7F, 0x80, 0x81, 0xFE, 0xFF]
    halves = np.array([h << 8 | l for h in edge for l in edge],
                      dtype=np.uint32)
    words = (halves[:, None] << 16 | halves[None, :]).reshape(-1)
    assert words.size == 2401
    _check_digits(words.astype(np.int32))


@gpu
@pytest.mark.parametrize("count", [1, 100003])
def test_digit_planes_random(count):
    # 100003 is no multiple of 256: the last block is partly idle
    rng = np.random.default_rng(count)
    _check_digits(_random(rng, (count,)))


@gpu
def test_digit_planes_grid_stride():
    """launch_digits caps the grid at 2^20 blocks of 256, so past 2^28
    words each thread loops; a 2 GiB table (2^29 words) gets there.
    2^28 + 257 words is the smallest count at which a second block's
    threads take a second trip.  Input, kernel output (1 GiB each) and the
    sliced reference stay on the device."""
    count = (1 << 28) + 257
    step = 1 << 24
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(28)
    x = torch.empty(count, dtype=torch.int32, device=dev)
    for lo in range(0, count, step):
        m = min(step, count - lo)
        x[lo:lo + m] = torch.randint(-(2**31), 2**31, (m,), dtype=torch.int64,
                                     device=dev, generator=g).to(torch.int32)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = ops._digit_planes(x)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for lo in range(0, count, step):
        hi = min(count, lo + step)
        v0 = x[lo:hi].to(torch.int64) & 0xFFFFFFFF
        v = v0
        total = torch.zeros_like(v0)
        for p in range(4):
            d = ((v + 128) & 0xFF) - 128
            got = out[p, lo:hi].to(torch.int64)
            bad += (got != d).sum()
            total += got << (8 * p)
            v = (v - d) >> 8
        bad += ((total & 0xFFFFFFFF) != v0).sum()
    n_bad = int(bad.item())
    print("digit planes, %d words: kernel %.3f s, check %.3f s" % (
        count, t1 - t0, time.perf_counter() - t1))
    assert n_bad == 0
    # the words only the second trip of the loop reaches
    _tail = x[1 << 28:].cpu().numpy()
    assert np.array_equal(out[:, 1 << 28:].cpu().numpy().astype(np.int64),
                          _ref_digits(_tail))
