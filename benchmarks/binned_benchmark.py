"""Batch-PIR serving step: one binned launch vs one launch per bin vs one
monolithic table.

A request sends one key to each of `num_bins` bins of `bin_n` rows; a step
serves `requests` of them, num_bins * requests keys.  Timed is the full
serving step (key H2D, kernel(s), share D2H) in three set-ups:

  binned  a BinnedDPF behind PipelinedServer: one fused launch per step in
          which every key walks its own bin
  loop    what the engine could do without it: num_bins DPF objects with
          one table each; one H2D of all keys, one eval_gpu_into per bin,
          one D2H of all shares
  mono    one DPF over the unbinned num_bins * bin_n rows behind
          PipelinedServer, same number of keys (each costs num_bins times
          the PRFs)
  packed  with --packed: a PackedBinnedDPF behind PipelinedServer over the
          same tables and slot plan, packed keys for the same rows (a
          quarter of the PRF blocks per key); needs --logn >= 9

Per set-up: warm-up steps, then `--windows` timed windows of at least
`--window-s` seconds each, all ending in a synchronise; the median window
is reported with the minimum and maximum.  `--entry-words` (16, 32, 48 or
64; default 16) is the row width of every table: wider than 16 words all
three set-ups run the wide fused kernel (fused_words).  The binned and loop shares are
compared once, exactly; packed shares differ from plain ones, so the packed
set-up is checked once by reconstructing the table rows from both servers'
packed shares, exactly.  One dict line per (config, set-up), then one per
config with the ratios (binned_over_packed with --packed); benchmarks/scrape.py reads them.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse
import statistics
import time

import torch

from gpudpf import BinnedDPF, DPF, PackedBinnedDPF
from gpudpf.serving import PipelinedServer


def rand_table(rows, seed, words=16):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, (rows, words), dtype=torch.int64,
                         generator=g).to(torch.int32)


def timed(step, drain, warmup, windows, window_s):
    """ms per step: median, min, max over the windows, and steps/window."""
    for _ in range(warmup):
        step()
    drain()
    torch.cuda.synchronize()
    per, steps = [], 0
    for _ in range(windows):
        steps = 0
        t0 = time.perf_counter()
        while steps < 20 or time.perf_counter() - t0 < window_s:
            step()
            steps += 1
        drain()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(per), min(per), max(per), steps


def pipelined(srv, keys):
    """(step, drain, last) keeping two batches in flight."""
    pending, last = [], [None]

    def step():
        pending.append(srv.submit(keys))
        if len(pending) == 2:
            last[0] = srv.collect(pending.pop(0))

    def drain():
        while pending:
            last[0] = srv.collect(pending.pop(0))

    return step, drain, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--logn", type=int, nargs="+", default=[12, 14])
    ap.add_argument("--requests", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prfs", nargs="+",
                    default=["AES128", "CHACHA20", "SALSA20"])
    ap.add_argument("--entry-words", type=int, default=16,
                    choices=list(DPF.FUSED_WIDTHS))
    ap.add_argument("--packed", action="store_true",
                    help="also time a PackedBinnedDPF (needs --logn >= 9)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("binned_benchmark needs a GPU")
    if a.packed and min(a.logn) < 9:
        raise SystemExit("--packed needs --logn >= 9 (packed domains start "
                         "at 512 rows)")
    dev = torch.device("cuda:0")

    for num_bins in a.bins:
        for logn in a.logn:
            n = 1 << logn
            tables = [rand_table(n, 100 * logn + b, a.entry_words)
                      for b in range(num_bins)]
            mono_table = torch.cat(tables)
            for prf_name in a.prfs:
                prf = getattr(DPF, "PRF_" + prf_name)
                binned = BinnedDPF(prf=prf, fused_words=a.entry_words)
                binned.eval_init(tables)
                loop = []
                for t in tables:
                    d = DPF(prf=prf, fused_words=a.entry_words)
                    d.eval_init(t)
                    loop.append(d)
                mono = DPF(prf=prf, fused_words=a.entry_words)
                mono.eval_init(mono_table)
                packed = None
                if a.packed:
                    packed = PackedBinnedDPF(prf=prf,
                                             fused_words=a.entry_words)
                    packed.eval_init(tables)
                for requests in a.requests:
                    run(a, dev, prf_name, num_bins, n, requests, binned,
                        loop, mono, packed)
                del binned, loop, mono, packed


def run(a, dev, prf_name, num_bins, n, requests, binned, loop, mono,
        packed=None):
    batch = num_bins * requests
    # `requests` consecutive slots per bin, so the per-bin loop takes slices
    plan = [b for b in range(num_bins) for _ in range(requests)]
    rows = [(i * 389 + 5) % n for i in range(batch)]
    keys, _ = binned.gen_batch(rows, plan)
    mono_keys, _ = mono.gen_batch(
        [b * n + r for b, r in zip(plan, rows)], num_bins * n)
    binned.bind_bins(plan)
    res = {}

    srv = PipelinedServer(binned, batch)
    step, drain, last = pipelined(srv, keys)
    res["binned"] = timed(step, drain, a.warmup, a.windows, a.window_s)
    binned_shares = last[0]
    del srv

    keys_pinned = keys.clone().pin_memory()
    keys_gpu = torch.zeros_like(keys, device=dev)
    out_gpu = torch.zeros((batch, a.entry_words), dtype=torch.int32,
                          device=dev)
    out_pinned = torch.zeros((batch, a.entry_words),
                             dtype=torch.int32).pin_memory()

    def loop_step():
        keys_pinned.numpy()[:] = keys.numpy()
        keys_gpu.copy_(keys_pinned, non_blocking=True)
        for b, d in enumerate(loop):
            lo = b * requests
            d.eval_gpu_into(keys_gpu[lo:lo + requests],
                            out_gpu[lo:lo + requests])
        out_pinned.copy_(out_gpu, non_blocking=True)
        torch.cuda.synchronize()

    res["loop"] = timed(loop_step, lambda: None, a.warmup, a.windows,
                        a.window_s)
    if not torch.equal(out_pinned, binned_shares):
        raise SystemExit("binned and per-bin shares differ")

    srv = PipelinedServer(mono, batch)
    step, drain, _last = pipelined(srv, mono_keys)
    res["mono"] = timed(step, drain, a.warmup, a.windows, a.window_s)
    del srv

    if packed is not None:
        pk1, pk2 = packed.gen_batch(rows, plan)
        packed.bind_bins(plan)
        srv = PipelinedServer(packed, batch)
        step, drain, last = pipelined(srv, pk1)
        res["packed"] = timed(step, drain, a.warmup, a.windows, a.window_s)
        other = srv.collect(srv.submit(pk2))
        rec = (last[0].to(torch.int64) - other.to(torch.int64)) \
            .to(torch.int32)
        want = torch.stack([packed.tables[b][r] for b, r in zip(plan, rows)])
        if not torch.equal(rec, want):
            raise SystemExit("packed shares do not reconstruct the rows")
        del srv

    cfg = {"prf": prf_name, "num_bins": num_bins, "bin_n": n,
           "entry_words": a.entry_words, "requests": requests, "keys": batch}
    for setup, (med, lo, hi, steps) in res.items():
        print(dict(cfg, setup=setup, ms_per_step=round(med, 4),
                   ms_min=round(lo, 4), ms_max=round(hi, 4),
                   steps_per_window=steps,
                   keys_per_sec=round(batch / med * 1e3, 1)), flush=True)
    summary = dict(
        cfg, setup="summary",
        binned_ms=round(res["binned"][0], 4),
        loop_ms=round(res["loop"][0], 4),
        mono_ms=round(res["mono"][0], 4),
        loop_over_binned=round(res["loop"][0] / res["binned"][0], 2),
        mono_over_binned=round(res["mono"][0] / res["binned"][0], 2))
    if packed is not None:
        summary["packed_ms"] = round(res["packed"][0], 4)
        summary["binned_over_packed"] = round(
            res["binned"][0] / res["packed"][0], 2)
    print(summary, flush=True)


if __name__ == "__main__":
    main()
