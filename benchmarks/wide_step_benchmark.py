"""Kernel step times of the three ways to serve a table: the 16-word fused
kernel, two-stage on rows of 32 / 64 words, and the wide fused kernel
(DPF(fused_words=64)) on the same rows.

Keys are resident on the device and nothing is copied per step: a fused step
is out.zero_() plus one DPF._launch_fused, a two-stage step is
DPF._eval_gpu_two_stage.  Per timing 3 warm-up steps, then `--windows`
windows of at least `--window-s` seconds, synchronising every 8 steps; the
median window is reported with the minimum and maximum.
The fused-wide shares are compared with the two-stage shares of the same
keys, exactly, before anything is timed.  Timing needs no host table, so the
device tables are allocated with eval_init_empty and filled with random
words in place.  One dict line per timing; lines starting with # are
progress stamps.

Copied into a checkout from before fused_words existed it still runs, and
prints the fused16 and two_stage rows only.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse
import inspect
import statistics
import time

import torch

from gpudpf import DPF

HAS_WIDE = "fused_words" in inspect.signature(DPF.__init__).parameters
T0 = time.perf_counter()
SYNC_EVERY = 8


def stamp(what):
    torch.cuda.synchronize()
    print("# %7.1fs %s" % (time.perf_counter() - T0, what), flush=True)


def timed(step, windows, window_s):
    """ms per step: median, min, max over the windows.  Steps are enqueued
    SYNC_EVERY at a time, so the launch queue stays short (an unbounded
    queue holds minutes of work) and the synchronise costs at most 1/8 of
    a launch latency per step."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        steps = 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < window_s:
            for _ in range(SYNC_EVERY):
                step()
            torch.cuda.synchronize()
            steps += SYNC_EVERY
        per.append((time.perf_counter() - t0) / steps * 1e3)
    return statistics.median(per), min(per), max(per)


def fused_step(dpf, keys_gpu):
    out = torch.zeros((len(keys_gpu), dpf._entry_padded), dtype=torch.int32,
                      device=keys_gpu.device)

    def step():
        out.zero_()
        dpf._launch_fused(keys_gpu, out)

    return step, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--prfs", nargs="+", default=["AES128", "CHACHA20"])
    ap.add_argument("--entry-words", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--tag", default="here",
                    help="copied into every line (which checkout ran)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_step_benchmark needs a GPU")
    for prf_name in a.prfs:
        prf = getattr(DPF, "PRF_" + prf_name)
        for logn in a.logn:
            n = 1 << logn
            keys = None
            stamp("start %s 2^%d" % (prf_name, logn))
            for ep in a.entry_words:
                # timing needs no host table: allocate the device table and
                # fill it with random words in place (any row order will do)
                dpf = DPF(prf=prf)
                dpf.eval_init_empty(n, ep)
                stamp("alloc %d done" % ep)
                g = torch.Generator(device=dpf._table_gpu.device)
                g.manual_seed(logn * 100 + ep)
                dpf._table_gpu.copy_(torch.randint(
                    -(2**31), 2**31, dpf._table_gpu.shape, dtype=torch.int64,
                    generator=g, device=dpf._table_gpu.device))
                stamp("fill %d done" % ep)
                if keys is None:
                    keys, _ = dpf.gen_batch(
                        [(i * 7919 + 3) % n for i in range(a.batch)], n)
                keys_gpu = keys.to(dpf._table_gpu.device)
                rows = {}
                if ep == 16:
                    step, _out = fused_step(dpf, keys_gpu)
                    rows["fused16"] = step
                else:
                    ref = dpf._eval_gpu_two_stage(keys_gpu)
                    stamp("two_stage ref done")
                    rows["two_stage"] = \
                        lambda: dpf._eval_gpu_two_stage(keys_gpu)
                    if HAS_WIDE:
                        wide = DPF(prf=prf, fused_words=64)
                        wide.eval_init_empty(n, ep)
                        wide._table_gpu.copy_(dpf._table_gpu)
                        stamp("wide table done")
                        step, out = fused_step(wide, keys_gpu)
                        step()
                        torch.cuda.synchronize()
                        if not torch.equal(out, ref):
                            raise SystemExit("fused_wide != two_stage")
                        rows["fused_wide"] = step
                for name, step in rows.items():
                    med, lo, hi = timed(step, a.windows, a.window_s)
                    print(dict(tree=a.tag, path=name, prf=prf_name, logn=logn,
                               ep=ep, batch=a.batch, ms=round(med, 4),
                               ms_min=round(lo, 4), ms_max=round(hi, 4)),
                          flush=True)
                del dpf, rows
                stamp("timed %d done" % ep)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
