"""Huge-table PIR serving benchmark — the 288 GB/GPU HBM3E story
(BASELINE config 5 on a single MI355X).

The table is built directly in HBM (eval_init_empty + chunked on-GPU
fill with a seeded generator) and NEVER exists on the host; DPF
reconstruction is verified against table_read before timing.  (The exact
single-server check at large offsets is tests/test_gpu_large_offsets.py.)

Shapes:
  wide      n=2^28, e=224 u32  -> 240.5 GB table, two-stage streaming-GEMM
  deep      n=2^30, e=16       ->  68.7 GB, fused path
  deep32    n=2^32, e=16       -> 274.9 GB, fused path (depth-32 keys,
                                  the wire-format maximum)

Emits one dict line per run: ms/step, DPFs/sec, and the effective table
bandwidth of the timed path.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse
import time

import torch

from gpudpf import DPF, _core

SHAPES = {
    "wide": (28, 224),
    "deep": (30, 16),
    "deep32": (32, 16),
    "smoke": (20, 64),   # tiny variant so the script itself is testable
}


def fill_rows(n, e, chunk_rows, seed, device):
    """Deterministic on-GPU synthetic rows: chunk c is regenerable."""
    for lo in range(0, n, chunk_rows):
        hi = min(n, lo + chunk_rows)
        g = torch.Generator(device=device)
        g.manual_seed(seed + lo)
        rows = torch.randint(-(2**31), 2**31 - 1, (hi - lo, e),
                             dtype=torch.int32, device=device, generator=g)
        yield lo, hi, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=list(SHAPES), default="wide")
    ap.add_argument("--batch", type=int, default=0,
                    help="0 = per-shape default (wide 8 / deep 8 / "
                         "deep32 4 / smoke 64)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--prf", default="CHACHA20")
    ap.add_argument("--checks", type=int, default=4)
    ap.add_argument("--pipeline", action="store_true",
                    help="pipelined wide serving (TwoStageServer)")
    args = ap.parse_args()

    log_n, e = SHAPES[args.shape]
    n = 1 << log_n
    if args.batch == 0:
        args.batch = {"wide": 8, "deep": 8, "deep32": 4, "smoke": 64}[
            args.shape]
    prf = getattr(DPF, "PRF_" + args.prf)
    dev = "cuda:0"
    table_gb = n * e * 4 / 1e9

    d = DPF(prf=prf, device=dev)
    t0 = time.time()
    d.eval_init_empty(n, e)
    chunk_rows = max(1, (1 << 30) // (e * 4))  # 1 GiB fill chunks
    seed = 20260914
    for lo, hi, rows in fill_rows(n, e, chunk_rows, seed, dev):
        d.table_write(torch.arange(lo, hi), rows)
        del rows
    torch.cuda.synchronize()
    t_fill = time.time() - t0
    free, total = torch.cuda.mem_get_info()
    print({"event": "filled", "table_gb": round(table_gb, 1),
           "fill_s": round(t_fill, 1),
           "hbm_used_gb": round((total - free) / 1e9, 1)})

    # correctness: DPF reconstruction at random indices == stored rows
    g = torch.Generator().manual_seed(7)
    alphas = [int(torch.randint(0, n, (1,), generator=g).item())
              for _ in range(args.checks)]
    stored = d.table_read(torch.tensor(alphas, dtype=torch.int64)).cpu()
    for ci, alpha in enumerate(alphas):
        k1, k2 = d.gen(alpha, n)
        a = d.eval_gpu([k1]).to(torch.int64)
        b = d.eval_gpu([k2]).to(torch.int64)
        rec = (a - b).to(torch.int32)[0]
        assert torch.equal(rec, stored[ci]), (
            "reconstruction mismatch at alpha=%d" % alpha)
    print({"event": "verified", "checks": args.checks})

    # serving benchmark
    ks, _ = _core.gen_batch(
        torch.randint(0, n, (args.batch,), generator=g).numpy(),
        n, b"huge-bench", prf)
    keys = torch.from_numpy(ks)
    ep = -(-e // 16) * 16
    if args.pipeline and ep > 16 and args.batch <= 16:
        # pipelined wide serving: expansion of step i+1 under the GEMM
        # of step i (every step still does its full work)
        from gpudpf.serving import TwoStageServer

        srv = TwoStageServer(d, args.batch)
        pending = []

        def step():
            pending.append(srv.submit(keys))
            if len(pending) >= 2:
                srv.collect(pending.pop(0))

        def drain():
            while pending:
                srv.collect(pending.pop(0))
    else:
        def step():
            d.eval_gpu(keys)

        def drain():
            pass
    for _ in range(args.warmup):
        step()
    drain()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.steps):
        step()
    drain()
    torch.cuda.synchronize()
    dt = (time.time() - t0) / args.steps
    # unambiguous lower bound on the table streaming rate: every step
    # reads the full padded table at least once (the two-stage GEMM
    # streams it once per 16-key chunk; the fused path once per key with
    # cross-key L2 reuse on top)
    one_pass_gbps = (1 << log_n) * ep * 4 / dt / 1e9
    print({"shape": args.shape, "n": n, "entry_words": e,
           "table_gb": round(table_gb, 1), "prf": args.prf,
           "batch": args.batch, "ms_per_step": round(dt * 1e3, 2),
           "dpfs_per_sec": round(args.batch / dt, 1),
           "table_gbps_one_pass_lower_bound": round(one_pass_gbps, 1)})


if __name__ == "__main__":
    main()
