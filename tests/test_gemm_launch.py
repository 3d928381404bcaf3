"""The GEMMs' launch layer: the three K-split queries against an independent
restatement of their arithmetic, the launchers' argument checks (made before
any HIP call, so they run on a machine without a GPU) and the argument
checks of gpudpf.ops; on the GPU, the launches that must leave memory
untouched."""

import pytest
import torch

from gpudpf import ops

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

needs_hip = pytest.mark.skipif(_hip is None,
                               reason="gpudpf._hip cannot be imported")
gpu = pytest.mark.gpu

KS = [1, 63, 64, 65, 127, 128, 192, 4096, 4099, 8192, 8256, 16448,
      (1 << 20) + 1, (1 << 28) + 65]
NS = [1, 5, 15, 16, 17, 255, 256, 257, 258, 4096, 1 << 20]
MS = [1, 15, 16, 17, 64, 1000, 1 << 16]
BATCHES = [1, 4, 5, 8, 9, 16]
POISON = 0x5A5A5A5A


def c(a, b):
    return -(-a // b)


def r64(a):
    return c(a, 64) * 64


def pow2_split(K, want):
    s = 1
    while s * 2 <= want and s * 2 <= c(K, 64):
        s *= 2
    return s, r64(c(K, s))


def gemm128_restated(M, N, K):
    return pow2_split(K, c(4096, c(M, 16) * c(N, 16)))


def mfma_restated(M, N, K):
    return pow2_split(K, c(1024, (M // 64) * (N // 16)))


def stream_restated(batch, K, N):
    segs = min(c(4096, c(N, 256)), c(K, 64))
    cap = (1 << 30) // (batch * N * 4)
    if cap >= 1:
        segs = min(segs, cap)
    segs = max(segs, 1)
    kchunk = r64(c(K, segs))
    return c(K, kchunk), kchunk


def _check_cover(split, K, tag):
    segs, kchunk = split
    assert segs >= 1, tag
    assert kchunk % 64 == 0, tag
    assert segs * kchunk >= K, tag


# ----------------------------------------------------------------------
# the K-splits (host arithmetic, no GPU)
# ----------------------------------------------------------------------
@needs_hip
def test_gemm128_split_covers_k():
    for M in MS:
        for N in NS:
            for K in KS:
                got = _hip.gemm128_split(M, N, K)
                _check_cover(got, K, (M, N, K, got))
                assert got == gemm128_restated(M, N, K), (M, N, K)
    assert _hip.gemm128_split(16, 16, 8256) == (128, 128)


@needs_hip
def test_gemm_u32_split_matches_restatement():
    for M in [64, 128, 512, 4096, 1 << 16]:
        for N in sorted({c(n, 16) * 16 for n in NS}):
            for K in sorted({r64(k) for k in KS}):
                got = _hip.gemm_u32_split(M, N, K)
                _check_cover(got, K, (M, N, K, got))
                assert got == mfma_restated(M, N, K), (M, N, K)


@needs_hip
def test_gemm_u32_stream_split_covers_k():
    for batch in BATCHES:
        for N in NS:
            for K in KS:
                got = _hip.gemm_u32_stream_split(batch, K, N)
                tag = (batch, K, N, got)
                _check_cover(got, K, tag)
                segs, kchunk = got
                assert (segs - 1) * kchunk < K, tag  # no empty last slice
                if batch * N * 4 <= 1 << 30:
                    assert segs * batch * N * 4 <= 1 << 30, tag
                assert got == stream_restated(batch, K, N), tag
    # 64 slices of 64 rows and a last one of 3
    assert _hip.gemm_u32_stream_split(3, 4099, 64) == (65, 64)


@needs_hip
@pytest.mark.parametrize("args", [(0, 1, 1), (1, 0, 1), (1, 1, 0),
                                  (-1, 16, 64)])
def test_gemm128_split_rejects_empty_shapes(args):
    with pytest.raises(ValueError):
        _hip.gemm128_split(*args)


@needs_hip
@pytest.mark.parametrize("args", [(0, 64, 16), (17, 64, 16), (-1, 64, 16),
                                  (1, 0, 16), (1, 64, 0), (1, -64, 16)])
def test_gemm_u32_stream_split_rejects(args):
    with pytest.raises(ValueError):
        _hip.gemm_u32_stream_split(*args)


# ----------------------------------------------------------------------
# the launchers reject bad arguments before any HIP call (no GPU): a
# RuntimeError "HIP error" here would mean a HIP call came first
# ----------------------------------------------------------------------
P = 0x1000  # a non-null "pointer"; nothing dereferences it


@needs_hip
@pytest.mark.parametrize("args", [
    (P, P, P, P, 1 << 30, 0, 16, 64), (P, P, P, P, 1 << 30, 16, 0, 64),
    (P, P, P, P, 1 << 30, 16, 16, 0), (P, P, P, P, 1 << 30, 16, 16, -64),
    (0, P, P, P, 1 << 30, 16, 16, 64), (P, 0, P, P, 1 << 30, 16, 16, 64),
    (P, P, 0, P, 1 << 30, 16, 16, 64), (P, P, P, 0, 1 << 30, 16, 16, 64),
    (P, P, P, P, 16 * 16 * 16 - 1, 16, 16, 64),       # segs = 1
    (P, P, P, P, 128 * 16 * 16 * 16 - 16, 16, 16, 8256),  # one u128 short
    (P, P, P, P, 0, 1, 1, 1),
], ids=str)
def test_launch_gemm128_rejects(args):
    with pytest.raises(ValueError):
        _hip.gemm128(*args, 0)


@needs_hip
@pytest.mark.parametrize("args", [
    (0, P, P, 64, 16, 64), (P, 0, P, 64, 16, 64), (P, P, 0, 64, 16, 64),
    (P, P, P, 0, 16, 64), (P, P, P, 64, 0, 64), (P, P, P, 64, 16, 0),
    (P, P, P, 63, 16, 64),
], ids=str)
def test_launch_gemm_u32_mfma_rejects(args):
    with pytest.raises(ValueError):
        _hip.gemm_u32_mfma(*args, 0)


@needs_hip
@pytest.mark.parametrize("args", [
    (P, P, P, 0, 64, 16), (P, P, P, 17, 64, 16), (P, P, P, 1, 0, 16),
    (P, P, P, 1, 64, 0), (P, P, P, 1, -1, 16), (P, P, P, 1, 64, -1),
    (P, P, P, 1, 64, 65535 * 256 + 1),  # 65536 column tiles
    (0, P, P, 1, 64, 16), (P, 0, P, 1, 64, 16), (P, P, 0, 1, 64, 16),
], ids=str)
def test_launch_gemm_u32_stream_rejects(args):
    with pytest.raises(ValueError):
        _hip.gemm_u32_stream(*args, 0)


@needs_hip
@pytest.mark.parametrize("args", [(P, P, -1), (0, P, 1), (P, 0, 1),
                                  (0, 0, 256)], ids=str)
def test_launch_digits_rejects(args):
    with pytest.raises(ValueError):
        _hip.digits(*args, 0)


@needs_hip
def test_launch_digits_of_nothing_launches_nothing():
    """count == 0 returns before any HIP call, null pointers or not."""
    _hip.digits(0, 0, 0, 0)


# ----------------------------------------------------------------------
# gpudpf.ops checks dtype, rank and agreeing shapes before anything moves
# to the device: CPU tensors, no GPU needed
# ----------------------------------------------------------------------
def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


@needs_hip
@pytest.mark.parametrize("fn", [ops.pir_matmul_u32, ops.pir_matmul_u32_stream])
def test_ops_matmul_rejects(fn):
    with pytest.raises(Exception, match="shares must be int32"):
        fn(_i32(2, 64).to(torch.int64), _i32(64, 16))
    with pytest.raises(Exception, match="table must be int32"):
        fn(_i32(2, 64), _i32(64, 16).to(torch.float32))
    with pytest.raises(Exception, match="must be 2-D"):
        fn(_i32(64), _i32(64, 16))
    with pytest.raises(Exception, match="must be 2-D"):
        fn(_i32(2, 64), _i32(64, 16, 1))
    with pytest.raises(Exception, match="disagree on K"):
        fn(_i32(2, 64), _i32(65, 16))


@needs_hip
def test_ops_stream_rejects_bad_out():
    a, b = _i32(2, 64), _i32(64, 16)
    for out in [_i32(2, 15), _i32(3, 16), _i32(2, 16).to(torch.int64),
                _i32(16, 2).t(),  # non-contiguous
                _i32(2, 16)]:     # right, but not where the GEMM runs
        with pytest.raises(Exception, match="out must be a contiguous"):
            ops.pir_matmul_u32_stream(a, b, out=out)


@needs_hip
def test_ops_gemm128_rejects():
    with pytest.raises(Exception, match="a must be int32"):
        ops.gemm128(_i32(2, 8, 4).to(torch.int64), _i32(3, 8, 4))
    with pytest.raises(Exception, match="bt must be int32"):
        ops.gemm128(_i32(2, 8, 4), _i32(3, 8, 4).to(torch.int16))
    with pytest.raises(Exception, match=r"must be \[M,K,4\]"):
        ops.gemm128(_i32(2, 8), _i32(3, 8, 4))
    with pytest.raises(Exception, match=r"must be \[M,K,4\]"):
        ops.gemm128(_i32(2, 8, 4), _i32(3, 8, 2))
    with pytest.raises(Exception, match="disagree on K"):
        ops.gemm128(_i32(2, 8, 4), _i32(3, 9, 4))


@needs_hip
def test_ops_launch_functions_check_tensors():
    """The private launch functions check every tensor against the shapes
    the others imply, before the current device is looked at."""
    a, b = _i32(2, 64), _i32(64, 16)
    with pytest.raises(Exception, match="c must be a contiguous"):
        ops._launch_gemm_stream(a, b, _i32(2, 15))
    with pytest.raises(Exception, match="a must be a contiguous"):
        ops._launch_gemm_stream(_i32(64, 2).t(), b, _i32(2, 16))
    with pytest.raises(Exception, match="planes must be a contiguous"):
        ops._launch_digits(_i32(10), torch.zeros((4, 9), dtype=torch.int8))
    with pytest.raises(Exception, match="dbt must be a contiguous"):
        ops._launch_gemm_mfma(torch.zeros((4, 64 * 64), dtype=torch.int8),
                              torch.zeros((4, 16 * 63), dtype=torch.int8),
                              _i32(64, 16), 64)
    with pytest.raises(Exception, match="partials must be a contiguous"):
        ops._launch_gemm128(_i32(16, 8256, 4), _i32(16, 8256, 4),
                            _i32(16, 16, 4), _i32(127, 16, 16, 4))


# ----------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------
@gpu
def test_launch_digits_of_nothing_leaves_output_untouched():
    dev = torch.device("cuda:0")
    x = torch.full((256,), POISON, dtype=torch.int32, device=dev)
    out = torch.full((4, 256), 0x5A, dtype=torch.int8, device=dev)
    _hip.digits(x.data_ptr(), out.data_ptr(), 0,
                torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert bool((out == 0x5A).all())
    assert ops._digit_planes(x[:0]).shape == (4, 0)


@gpu
def test_launch_gemm_stream_rejects_other_current_device():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    dev = torch.device("cuda:0")
    a = torch.ones((2, 64), dtype=torch.int32, device=dev)
    b = torch.ones((64, 16), dtype=torch.int32, device=dev)
    out = torch.full((2, 16), POISON, dtype=torch.int32, device=dev)
    with torch.cuda.device(1):
        with pytest.raises(Exception, match="current device is cuda:1"):
            ops._launch_gemm_stream(a, b, out)
    torch.cuda.synchronize(dev)
    assert bool((out == POISON).all())
