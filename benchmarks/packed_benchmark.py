"""Serving step with packed keys vs plain keys, same table, same indices.

A step serves `--batch` keys against one table of n rows of 16 words behind
PipelinedServer: key H2D, one fused launch, share D2H, two batches in
flight.  Two set-ups on the same seeded table and the same secret indices:

  plain   DPF: 2n - 2 PRF blocks per key, one u32 leaf per block
  packed  PackedDPF: n/2 - 2 blocks per key, four u32 leaves per block

They alternate in one process: window 1 plain, window 1 packed, window 2
plain, ...  Each of the `--windows` timed windows runs at least
`--window-s` seconds and ends in a synchronise; the median window is
reported with the minimum and maximum.  Beside each time stands the table
delivery rate it implies, batch * n * 64 B / step: every key reads every
row once, from wherever the rows happen to live.  The packed
reconstruction is compared with the plain one once per config, exactly.
One dict line per (config, set-up), then one per config with the ratio;
benchmarks/scrape.py reads them.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse
import statistics
import time

import torch

from gpudpf import DPF, PackedDPF
from gpudpf.serving import PipelinedServer

from binned_benchmark import pipelined, rand_table


def window(step, drain, window_s):
    """ms per step over one window of at least window_s seconds."""
    steps = 0
    t0 = time.perf_counter()
    while steps < 20 or time.perf_counter() - t0 < window_s:
        step()
        steps += 1
    drain()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, steps


def timed_alternating(setups, warmup, windows, window_s):
    """{name: (median, min, max, steps)} with the set-ups' windows
    interleaved; setups is {name: (step, drain)}."""
    for step, drain in setups.values():
        for _ in range(warmup):
            step()
        drain()
    torch.cuda.synchronize()
    per = {name: [] for name in setups}
    steps = {}
    for _ in range(windows):
        for name, (step, drain) in setups.items():
            ms, steps[name] = window(step, drain, window_s)
            per[name].append(ms)
    return {name: (statistics.median(v), min(v), max(v), steps[name])
            for name, v in per.items()}


def sub(a, b):
    return (a.to(torch.int64) - b.to(torch.int64)).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="+", default=[14, 16, 18, 20])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--prfs", nargs="+",
                    default=["AES128", "CHACHA20", "SALSA20"])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=3.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("packed_benchmark needs a GPU")

    for logn in a.logn:
        n = 1 << logn
        table = rand_table(n, 4000 + logn)
        rows = [(i * 389 + 5) % n for i in range(a.batch)]
        want = table[rows]
        for prf_name in a.prfs:
            prf = getattr(DPF, "PRF_" + prf_name)
            engines = {"plain": DPF(prf=prf), "packed": PackedDPF(prf=prf)}
            setups, lasts, keys2 = {}, {}, {}
            for name, d in engines.items():
                d.eval_init(table)
                k1s, k2s = d.gen_batch(rows, n)
                keys2[name] = k2s
                srv = PipelinedServer(d, a.batch)
                step, drain, last = pipelined(srv, k1s)
                setups[name], lasts[name] = (step, drain), last
            res = timed_alternating(setups, a.warmup, a.windows, a.window_s)
            # one exact check: both reconstruct the same rows
            recs = {name: sub(lasts[name][0], engines[name].eval_gpu(keys2[name]))
                    for name in engines}
            if not (torch.equal(recs["plain"], want)
                    and torch.equal(recs["packed"], recs["plain"])):
                raise SystemExit("packed and plain reconstructions differ")

            cfg = {"prf": prf_name, "n": n, "entry_words": 16,
                   "keys": a.batch}
            table_bytes = a.batch * n * 64
            for name, (med, lo, hi, steps) in res.items():
                print(dict(cfg, setup=name, ms_per_step=round(med, 4),
                           ms_min=round(lo, 4), ms_max=round(hi, 4),
                           steps_per_window=steps,
                           keys_per_sec=round(a.batch / med * 1e3, 1),
                           table_tb_per_s=round(table_bytes / med / 1e9, 3)),
                      flush=True)
            p, q = res["plain"], res["packed"]
            print(dict(cfg, setup="summary", plain_ms=round(p[0], 4),
                       packed_ms=round(q[0], 4),
                       plain_over_packed=round(p[0] / q[0], 2),
                       packed_max_below_plain_min=q[2] < p[1],
                       packed_table_tb_per_s=round(
                           table_bytes / q[0] / 1e9, 3)), flush=True)
            del setups, lasts, engines


if __name__ == "__main__":
    main()
