"""From a batch-PIR plan to something the engine serves.

A BatchPIROptimize hashes the cold groups of a table into `num_bins` bins
and budgets `queries_per_bin` PIR queries per bin and request.  This module
lays the bins out as tables for gpudpf.BinnedDPF, builds the fixed slot plan
of a request, makes the client's keys for it and decodes the two servers'
answers:

    tables = bin_tables(opt, table)           # server: one table per bin
    dpf.eval_init(tables)
    dpf.bind_bins(slot_bins(opt))             # same plan for every request
    k1s, k2s, meaning = make_queries(opt, dpf, indices)      # client
    a, b = server1(k1s), server2(k2s)         # [slots, group_size * e] each
    rows = decode(opt, meaning, a, b, e)      # {cold entry: its row}

A collocated plan's rows are group_size * e words.  Beyond 16 words pass the
width limit on both sides (at most 64):

    tables = bin_tables(opt, table, max_words=64)
    dpf = BinnedDPF(fused_words=64)

gpudpf.PackedBinnedDPF takes BinnedDPF's place on both sides unchanged (same
tables, same slot plan, same decode; its keys are packed, a quarter of the
PRF work per key, and neither engine accepts the other's):

    dpf = PackedBinnedDPF(fused_words=64)

Every request issues num_bins * queries_per_bin keys in the same slot
order whatever it asks for, so the servers learn nothing from which bins
were needed.
"""

import collections

import torch

ENTRY_WORDS = 16  # widest row a default BinnedDPF (fused_words=16) serves


def _group_size(opt):
    return max(1, int(opt.collocate.group_size))


def _bin_groups(opt, b):
    """Group ids of bin b in table-row order (ascending)."""
    return sorted(opt.bins.get(b, []))


def bin_tables(opt, table, max_words=ENTRY_WORDS):
    """The per-bin tables of plan `opt` over `table` ([num_entries, e]
    int32): row r of bin b is the concatenation of the rows of the entries
    of group sorted(opt.bins[b])[r], zero-padded to group_size * e words.
    A bin the hash left empty gets one zero row, so every bin exists.
    max_words is the fused_words of the BinnedDPF that will serve them."""
    e = int(table.shape[1])
    width = _group_size(opt) * e
    if width > max_words:
        raise Exception("group_size * e = %d words, but a binned row holds "
                        "at most %d" % (width, max_words))
    t32 = table.to(torch.int32)
    out = []
    for b in range(opt.pir.num_bins):
        gids = _bin_groups(opt, b)
        bt = torch.zeros((max(1, len(gids)), width), dtype=torch.int32)
        for r, gid in enumerate(gids):
            members = opt.groups[gid]
            bt[r, : len(members) * e] = t32[members].reshape(-1)
        out.append(bt)
    return out


def slot_bins(opt):
    """The fixed slot plan of every request: queries_per_bin consecutive
    slots per bin."""
    return [b for b in range(opt.pir.num_bins)
            for _ in range(opt.pir.queries_per_bin)]


def make_queries(opt, dpf, indices):
    """Client side: the keys of one request for `indices`.

    Makes the greedy choice of opt.fetch (most-requested groups first, at
    most queries_per_bin per bin); idle slots get a dummy key for row 0.
    `dpf` is a BinnedDPF or PackedBinnedDPF that knows the bin sizes (any
    engine with gen_batch(rows, bins)); the keys are of its kind.  Returns (k1s, k2s,
    slot_meaning): slot_meaning[s] is None for an idle slot, else
    (group id, the requested entries of that group)."""
    q = opt.pir.queries_per_bin
    want = set(indices)
    needed = collections.Counter()
    for i in want:
        if i not in opt.hot_set:
            needed[opt.group_of[i]] += 1
    per_bin = collections.defaultdict(list)
    for gid, cnt in needed.items():
        per_bin[opt.bin_of[gid]].append((cnt, gid))
    rows, meaning = [], []
    for b in range(opt.pir.num_bins):
        row_of = {gid: r for r, gid in enumerate(_bin_groups(opt, b))}
        chosen = sorted(per_bin.get(b, []), reverse=True)[:q]
        for _cnt, gid in chosen:
            rows.append(row_of[gid])
            meaning.append(
                (gid, tuple(x for x in opt.groups[gid] if x in want)))
        for _ in range(q - len(chosen)):
            rows.append(0)
            meaning.append(None)
    k1s, k2s = dpf.gen_batch(rows, slot_bins(opt))
    return k1s, k2s, meaning


def decode(opt, slot_meaning, a, b, e):
    """{entry index: its e-word row} for the cold entries a request
    recovered, from the two servers' shares a, b ([slots, >= group_size * e]
    int32)."""
    rec = (a.to(torch.int64) - b.to(torch.int64)).to(torch.int32)
    out = {}
    for s, m in enumerate(slot_meaning):
        if m is None:
            continue
        gid, wanted = m
        members = opt.groups[gid]
        for x in wanted:
            pos = members.index(x)
            out[x] = rec[s, pos * e:(pos + 1) * e].clone()
    return out
