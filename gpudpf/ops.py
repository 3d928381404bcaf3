"""Standalone GPU ops (research-harness components).

The public functions check their arguments' dtype, rank and agreeing shapes
before anything moves to the device, and accept CPU tensors as a
convenience (`_gpu_device`).  Every kernel launch goes through a
`_launch_*` function, which checks each tensor (`_check_arg`) before its
raw pointer reaches a kernel."""

import torch

from gpudpf import _core
from gpudpf.dpf import _check_arg, _hip


def _require_i32(**tensors):
    for name, t in tensors.items():
        if t.dtype != torch.int32:
            raise Exception("%s must be int32 (got %s)" % (name, t.dtype))


def _require_matmul(shares, table):
    """shares [M,K] x table [K,N], both int32 -> (M, K, N)."""
    _require_i32(shares=shares, table=table)
    if shares.dim() != 2 or table.dim() != 2:
        raise Exception("shares and table must be 2-D (got %s and %s)"
                        % (list(shares.shape), list(table.shape)))
    if shares.shape[1] != table.shape[0]:
        raise Exception("shares [M,K] and table [K,N] disagree on K (%d, %d)"
                        % (shares.shape[1], table.shape[0]))
    return shares.shape[0], shares.shape[1], table.shape[1]


def _gpu_device(t):
    """Where `t`'s GEMM runs: its own device, cuda:0 for a CPU tensor."""
    return torch.device("cuda:0") if t.device.type == "cpu" else t.device


def _stream(dev):
    """The launch stream on `dev`, which must be the current device: the
    streaming GEMM's partials scratch belongs to the current device."""
    if torch.cuda.current_device() != dev.index:
        raise Exception("current device is cuda:%d but the tensors are on %s"
                        % (torch.cuda.current_device(), dev))
    return torch.cuda.current_stream(dev).cuda_stream


def _launch_gemm128(a, bt, c, partials):
    """c [M,N,4] = a [M,K,4] x bt [N,K,4] over Z_2^128; `partials` is the
    caller's [segs,M,N,4] K-split scratch."""
    dev, (M, K), N = a.device, a.shape[:2], bt.shape[0]
    segs = _hip.gemm128_split(M, N, K)[0]
    _check_arg("a", a, dev, torch.int32, (M, K, 4))
    _check_arg("bt", bt, dev, torch.int32, (N, K, 4))
    _check_arg("c", c, dev, torch.int32, (M, N, 4))
    _check_arg("partials", partials, dev, torch.int32, (segs, M, N, 4))
    _hip.gemm128(a.data_ptr(), bt.data_ptr(), c.data_ptr(),
                 partials.data_ptr(), partials.numel() * 4, M, N, K,
                 _stream(dev))


def _launch_digits(x, planes):
    """planes [4,count] int8 = the signed base-256 digits of x's `count`
    int32 words."""
    dev, count = x.device, x.numel()
    _check_arg("x", x, dev, torch.int32, x.shape)
    _check_arg("planes", planes, dev, torch.int8, (4, count))
    _hip.digits(x.data_ptr(), planes.data_ptr(), count, _stream(dev))


def _launch_gemm_mfma(da, dbt, c, K):
    """c [M,N] += A x B mod 2^32 from the digit planes da [4,M*K] of A [M,K]
    and dbt [4,N*K] of B transposed [N,K]; the caller zeroes c."""
    dev, (M, N) = c.device, c.shape
    _check_arg("da", da, dev, torch.int8, (4, M * K))
    _check_arg("dbt", dbt, dev, torch.int8, (4, N * K))
    _check_arg("c", c, dev, torch.int32, (M, N))
    _hip.gemm_u32_mfma(da.data_ptr(), dbt.data_ptr(), c.data_ptr(), M, N, K,
                       _stream(dev))


def _launch_gemm_stream(a, b, c):
    """c [batch,N] += a [batch,K] x b [K,N] mod 2^32, batch <= 16; the
    caller zeroes c."""
    dev, (batch, K), N = b.device, a.shape, b.shape[1]
    _check_arg("a", a, dev, torch.int32, (batch, K))
    _check_arg("b", b, dev, torch.int32, (K, N))
    _check_arg("c", c, dev, torch.int32, (batch, N))
    _hip.gemm_u32_stream(a.data_ptr(), b.data_ptr(), c.data_ptr(), batch, K,
                         N, _stream(dev))


def gemm128(a, bt):
    """Exact GEMM over Z_2^128: a [M,K,4] int32 (u128 little-endian limbs),
    bt [N,K,4] int32 -> [M,N,4] int32, computed on the GPU.

    This is the reference's standalone GEMM128 research kernel
    (dpf_gpu/matmul/matmul.cu) as a CDNA4 HIP kernel with K split across
    blockIdx.z and a mod-2^128 reduction kernel."""
    _require_i32(a=a, bt=bt)
    if (a.dim() != 3 or bt.dim() != 3 or a.shape[2] != 4
            or bt.shape[2] != 4):
        raise Exception("a and bt must be [M,K,4] and [N,K,4] (got %s and %s)"
                        % (list(a.shape), list(bt.shape)))
    if a.shape[1] != bt.shape[1]:
        raise Exception("a [M,K,4] and bt [N,K,4] disagree on K (%d, %d)"
                        % (a.shape[1], bt.shape[1]))
    M, K = a.shape[0], a.shape[1]
    N = bt.shape[0]
    dev = _gpu_device(a)
    c_g = torch.empty((M, N, 4), dtype=torch.int32, device=dev)
    segs = _hip.gemm128_split(M, N, K)[0]
    scratch = torch.empty((segs, M, N, 4), dtype=torch.int32, device=dev)
    _launch_gemm128(a.to(dev).contiguous(), bt.to(dev).contiguous(), c_g,
                    scratch)
    return c_g


def gemm128_cpu(a, bt):
    """CPU reference for gemm128 (exact, single-threaded)."""
    import numpy as np

    return torch.from_numpy(
        np.asarray(_core.gemm128_cpu(a.numpy(), bt.numpy()))
    )


def _digit_planes(x_u32_gpu):
    """[..., count] int32 tensor on GPU -> [4, count] int8 signed base-256
    digit planes (flattened over the input shape)."""
    out = torch.empty((4, x_u32_gpu.numel()), dtype=torch.int8,
                      device=x_u32_gpu.device)
    _launch_digits(x_u32_gpu, out)
    return out


def pir_matmul_u32_stream(shares, table, out=None):
    """C = shares @ table mod 2^32, streaming the u32 table in place.

    shares: [M, K] int32, table: [K, N] int32 (both already on the GPU for
    the huge-table path).  Unlike pir_matmul_u32 this allocates NO copy of
    the table (no transpose, no digit planes) — the extra memory is the
    [M, N] output plus a <=1 GiB K-split partials scratch — so it serves
    tables sized to HBM capacity (200+ GB).  Batches > 16 are evaluated
    in 16-row chunks, each chunk re-streaming the table once: 16 is the
    bandwidth-bound register limit (4 uint4 accumulator sets per lane);
    re-streaming at the HBM line beats one instruction-bound pass, and
    genuinely compute-bound shapes belong to pir_matmul_u32 (MFMA)."""
    M, K, N = _require_matmul(shares, table)
    dev = _gpu_device(shares)
    if out is not None:
        _check_arg("out", out, dev, torch.int32, (M, N))
    a = shares.to(dev).contiguous()
    b = table.to(dev).contiguous()
    c = out if out is not None else torch.empty(
        (M, N), dtype=torch.int32, device=dev)
    for lo in range(0, M, 16):
        chunk = c[lo:lo + 16]
        chunk.zero_()
        _launch_gemm_stream(a[lo:lo + 16], b, chunk)
    return c


def pir_matmul_u32(shares, table):
    """C = shares @ table mod 2^32 on the MFMA matrix cores.

    shares: [M, K] int32 (e.g. one-hot DPF shares), table: [K, N] int32.
    Each u32 operand is decomposed into 4 signed base-256 digit planes and
    the product assembled from 10 i8-MFMA accumulator chains (see
    csrc/hip/gemm_u32.hip).  Exact mod 2^32.
    """
    M, K, N = _require_matmul(shares, table)
    dev = _gpu_device(shares)
    Mp, Np, Kp = -(-M // 64) * 64, -(-N // 16) * 16, -(-K // 64) * 64
    a = torch.zeros((Mp, Kp), dtype=torch.int32, device=dev)
    a[:M, :K] = shares.to(dev)
    bt = torch.zeros((Np, Kp), dtype=torch.int32, device=dev)
    bt[:N, :K] = table.to(dev).t()
    c = torch.zeros((Mp, Np), dtype=torch.int32, device=dev)
    _launch_gemm_mfma(_digit_planes(a), _digit_planes(bt), c, Kp)
    return c[:M, :N]
