"""How many LDS operations a kernel keeps in flight, read from its assembly.

Needs no GPU.  Input is a `.s` file from

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S ...

and a regular expression on the kernel's (mangled) name.  For every kernel
that matches it walks the wave's `lgkmcnt` counter down the instruction
stream in file order: every DS instruction and every scalar-memory load
increments it, an `s_waitcnt ... lgkmcnt(N)` clamps it to N.  Branches are
not followed, so the figures describe the straight-line text, which is what
matters for the unrolled cipher rounds that make up the AES kernels.

Printed per kernel:
  ds_read_b32     count of `ds_read_b32`
  waits           count of `s_waitcnt` that name lgkmcnt
  mean, peak      operations outstanding when a wait is reached (before the
                  clamp), and the most outstanding anywhere
  histogram       of the outstanding-at-wait values

    python benchmarks/lds_inflight.py dpf_eval.s 'dpf_eval_kernelILi3ELb1ELi4ELi1E'
"""

import argparse
import re
import sys

_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_END = re.compile(r"^\.Lfunc_end\d+:")
_WAIT = re.compile(r"^s_waitcnt\b(.*)$")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")
# instructions that count on lgkmcnt: LDS/GDS, scalar memory reads
_COUNTED = re.compile(r"^(ds_|s_load_|s_buffer_load_)")

# upper edges of the histogram buckets (inclusive); the last is open
BUCKETS = (0, 2, 4, 8, 16, 32)


def _bucket_labels():
    labels, lo = [], 0
    for hi in BUCKETS:
        labels.append(str(hi) if lo == hi else "%d-%d" % (lo, hi))
        lo = hi + 1
    labels.append("%d+" % lo)
    return labels


def _bucket(v):
    for i, hi in enumerate(BUCKETS):
        if v <= hi:
            return i
    return len(BUCKETS)


def kernels(text):
    """Yield (name, instruction lines) of every function in a .s text."""
    name, body = None, []
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if name is None:
            m = _LABEL.match(line)
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if _END.match(line):
            yield name, body
            name = None
            continue
        if line.startswith(".") or _LABEL.match(line):
            continue  # directives, block labels
        body.append(line)
    if name is not None:
        yield name, body


def walk(lines):
    """lgkmcnt walk over one kernel's instructions."""
    cnt = peak = reads = 0
    at_wait = []
    for line in lines:
        if _COUNTED.match(line):
            cnt += 1
            peak = max(peak, cnt)
            if line.startswith("ds_read_b32"):
                reads += 1
            continue
        m = _WAIT.match(line)
        if m:
            n = _LGKM.search(m.group(1))
            if n:
                at_wait.append(cnt)
                cnt = min(cnt, int(n.group(1)))
    hist = [0] * (len(BUCKETS) + 1)
    for v in at_wait:
        hist[_bucket(v)] += 1
    return {
        "ds_read_b32": reads,
        "waits": len(at_wait),
        "mean": sum(at_wait) / len(at_wait) if at_wait else 0.0,
        "peak": peak,
        "hist": hist,
    }


def analyse(text, pattern):
    """[(kernel name, walk() result)] for the kernels whose name matches."""
    rx = re.compile(pattern)
    return [(n, walk(b)) for n, b in kernels(text) if rx.search(n)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm", help=".s file")
    ap.add_argument("pattern", nargs="?", default=".",
                    help="regular expression on the mangled kernel name")
    args = ap.parse_args(argv)
    with open(args.asm) as f:
        found = analyse(f.read(), args.pattern)
    if not found:
        print("no kernel matches %r" % args.pattern, file=sys.stderr)
        return 1
    labels = _bucket_labels()
    for name, r in found:
        print(name)
        print("  ds_read_b32 %d  waits %d  mean outstanding at wait %.2f  "
              "peak %d" % (r["ds_read_b32"], r["waits"], r["mean"], r["peak"]))
        print("  at wait: " + "  ".join(
            "%s:%d" % (l, c) for l, c in zip(labels, r["hist"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
