"""GEMM128 tests: CPU reference self-consistency (vs python ints) and the
GPU kernel vs the CPU reference (the reference's 128-bit unit-test tier:
dpf_gpu/tests/test_128_bit.cu + matmul check).  The edge-shape tests check
the GPU kernel against python integers as well as against the CPU
reference, with random operands and with operands whose limbs sit on the
carry boundaries, and poison the K-split scratch before the launch."""

import functools

import numpy as np
import pytest
import torch

from gpudpf import ops

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

MASK128 = (1 << 128) - 1
# carries into, out of and across every 32- and 64-bit limb boundary
EXTREME = [0, 1, 2**32 - 1, 2**32, 2**64 - 1, 2**64, 2**127, 2**128 - 1]
# (17,15,65): ragged tiles on both axes, one-element last K stage;
# (16,16,8256): ksplit 128 with uneven slices, most of them empty
GPU_SHAPES = [(1, 1, 1), (16, 16, 64), (17, 15, 65), (3, 33, 63),
              (16, 16, 8256)]
POISONED = [(17, 15, 65), (16, 16, 8256)]
POISON = 0x5A5A5A5A


def _to_u128(arr):
    # [.,.,4] int32 LE limbs -> python int matrix
    a = arr.astype(np.uint32).astype(object)
    return a[..., 0] + (a[..., 1] << 32) + (a[..., 2] << 64) + (a[..., 3] << 96)


def _limbs(vals, shape):
    """python ints (flat, row-major) -> shape + (4,) int32 LE limbs."""
    out = np.empty((len(vals), 4), dtype=np.uint32)
    for i, v in enumerate(vals):
        for j in range(4):
            out[i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out.astype(np.int32).reshape(shape + (4,))


def _operands(kind, M, N, K):
    rng = np.random.default_rng(M * 1000003 + N * 1009 + K)
    if kind == "random":
        a = rng.integers(-(2**31), 2**31, (M, K, 4), dtype=np.int64)
        bt = rng.integers(-(2**31), 2**31, (N, K, 4), dtype=np.int64)
        return a.astype(np.int32), bt.astype(np.int32)
    ia = rng.integers(0, len(EXTREME), M * K)
    ib = rng.integers(0, len(EXTREME), N * K)
    return (_limbs([EXTREME[i] for i in ia], (M, K)),
            _limbs([EXTREME[i] for i in ib], (N, K)))


def _ref_python(a, bt):
    """[M,K,4] x [N,K,4] -> [M,N] python ints mod 2^128 (object-array dot:
    every multiply and add is a python integer operation)."""
    prod = np.dot(_to_u128(a), _to_u128(bt).T)
    return np.vectorize(lambda v: int(v) & MASK128, otypes=[object])(prod)


@functools.lru_cache(maxsize=None)
def _case(kind, M, N, K):
    """(a, bt, python-int reference); built once, never modified."""
    a, bt = _operands(kind, M, N, K)
    return a, bt, _ref_python(a, bt)


def test_gemm128_cpu_reference_exact():
    rng = np.random.default_rng(7)
    M, N, K = 3, 2, 5
    a = rng.integers(-(2**31), 2**31 - 1, (M, K, 4), dtype=np.int64).astype(np.int32)
    bt = rng.integers(-(2**31), 2**31 - 1, (N, K, 4), dtype=np.int64).astype(np.int32)
    got = ops.gemm128_cpu(torch.from_numpy(a), torch.from_numpy(bt)).numpy()
    av = _to_u128(a)
    bv = _to_u128(bt)
    mask = (1 << 128) - 1
    for m in range(M):
        for n in range(N):
            want = 0
            for k in range(K):
                want = (want + int(av[m, k]) * int(bv[n, k])) & mask
            gotv = int(_to_u128(got)[m, n])
            assert gotv == want


@pytest.mark.parametrize("M,N,K", [(3, 2, 5), (1, 1, 70)],
                         ids=lambda v: str(v))
def test_gemm128_cpu_reference_extreme_operands(M, N, K):
    a, bt = _operands("extreme", M, N, K)
    av, bv = _to_u128(a), _to_u128(bt)
    assert {int(v) for v in av.reshape(-1)} <= set(EXTREME)
    got = _to_u128(
        ops.gemm128_cpu(torch.from_numpy(a), torch.from_numpy(bt)).numpy())
    for m in range(M):
        for n in range(N):
            want = 0
            for k in range(K):
                want = (want + int(av[m, k]) * int(bv[n, k])) & MASK128
            assert int(got[m, n]) == want, (m, n)


@pytest.mark.gpu
def test_gemm128_gpu_matches_cpu():
    torch.manual_seed(3)
    for (M, N, K) in [(32, 16, 4096), (7, 5, 1000), (64, 16, 131072)]:
        a = torch.randint(-(2**31), 2**31 - 1, (M, K, 4), dtype=torch.int64).to(
            torch.int32
        )
        bt = torch.randint(-(2**31), 2**31 - 1, (N, K, 4), dtype=torch.int64).to(
            torch.int32
        )
        got = ops.gemm128(a, bt).cpu()
        want = ops.gemm128_cpu(a, bt)
        assert torch.equal(got, want), (M, N, K)


def _check_gpu(got, a, bt, want, tag):
    got = got.cpu()
    gotv = _to_u128(got.numpy())
    bad = [(m, n) for m in range(want.shape[0]) for n in range(want.shape[1])
           if int(gotv[m, n]) != want[m, n]]
    assert not bad, (tag, "%d of %d entries differ from python ints, "
                     "first at %s" % (len(bad), want.size, bad[0]))
    cpu = ops.gemm128_cpu(torch.from_numpy(a), torch.from_numpy(bt))
    assert torch.equal(got, cpu), tag


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("M,N,K", GPU_SHAPES, ids=lambda v: str(v))
def test_gemm128_gpu_edge_shapes(M, N, K, kind):
    if (M, N, K) == (16, 16, 8256):
        assert _hip.gemm128_split(M, N, K)[0] == 128
    a, bt, want = _case(kind, M, N, K)
    got = ops.gemm128(torch.from_numpy(a), torch.from_numpy(bt))
    _check_gpu(got, a, bt, want, (M, N, K, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("M,N,K", POISONED, ids=lambda v: str(v))
def test_gemm128_gpu_poisoned_scratch(M, N, K, kind):
    """The K-split partials start as 0x5A5A5A5A, so a slice the reduction
    reads without the GEMM having written it cannot pass for a sum."""
    a, bt, want = _case(kind, M, N, K)
    dev = torch.device("cuda:0")
    a_g = torch.from_numpy(a).to(dev)
    b_g = torch.from_numpy(bt).to(dev)
    ksplit = _hip.gemm128_split(M, N, K)[0]
    scratch = torch.full((ksplit, M, N, 4), POISON, dtype=torch.int32,
                         device=dev)
    c_g = torch.full((M, N, 4), POISON, dtype=torch.int32, device=dev)
    _hip.gemm128(a_g.data_ptr(), b_g.data_ptr(), c_g.data_ptr(),
                 scratch.data_ptr(), scratch.numel() * 4, M, N, K,
                 torch.cuda.current_stream(dev).cuda_stream)
    _check_gpu(c_g, a, bt, want, (M, N, K, kind))


@pytest.mark.gpu
def test_gemm128_gpu_rejects_short_partials():
    """Partials one u128 short of ksplit*M*N: nothing is launched."""
    M, N, K = 16, 16, 8256
    a, bt, _ = _case("random", M, N, K)
    dev = torch.device("cuda:0")
    a_g = torch.from_numpy(a).to(dev)
    b_g = torch.from_numpy(bt).to(dev)
    ksplit = _hip.gemm128_split(M, N, K)[0]
    assert ksplit == 128
    scratch = torch.full((ksplit * M * N - 1, 4), POISON, dtype=torch.int32,
                         device=dev)
    c_g = torch.full((M, N, 4), POISON, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        _hip.gemm128(a_g.data_ptr(), b_g.data_ptr(), c_g.data_ptr(),
                     scratch.data_ptr(), scratch.numel() * 4, M, N, K,
                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert bool((c_g == POISON).all()) and bool((scratch == POISON).all())
