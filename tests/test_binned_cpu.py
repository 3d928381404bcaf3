"""gpudpf.BinnedDPF and pir.serve on the host: layout, CPU reference,
every host-side rejection, and the planner round trip.  No GPU needed.

All comparisons are exact.  Bin tables are independently random, so a key
evaluated against the wrong bin cannot give the right share; each test
first shows that for its own keys (the share against the key's bin differs
from the share against bin 0).
"""

import functools
import random

import numpy as np
import pytest
import torch

from gpudpf import BinnedDPF, DPF, _core
from pir import BatchPIROptimize, CollocateConfig, HotColdConfig, PIRConfig
from pir import serve

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
SIZES = [1, 130, 77, 128, 5]       # unequal, not powers of two; domain 256
E = 5


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _tables(e=E):
    return tuple(_rand((n, e), 50 + b) for b, n in enumerate(SIZES))


def _engine(prf, e=E):
    d = BinnedDPF(prf=prf, device="cpu")
    d.eval_init(list(_tables(e)))
    return d


def _padded(t, n):
    p = np.zeros((n, 16), dtype=np.int32)
    p[: t.shape[0], : t.shape[1]] = t.numpy()
    return p


def test_layout_blocks_are_leaf_perm_of_padded_bins():
    d = _engine(DPF.PRF_SALSA20)
    assert d.num_bins == 5 and d.bin_sizes == SIZES
    assert d._n_domain == 256 and d._depth == 8
    assert d._zlog == _core.zlog_for_depth(8)
    assert d._entry_padded == 16 and d.table_effective_entry_size == E
    perm = _core.leaf_perm_table(256, d._zlog)
    assert sorted(perm.tolist()) == list(range(256))
    for b, t in enumerate(_tables()):
        blk = d.bin_block(b).numpy()
        assert blk.shape == (256, 16) and blk.dtype == np.int32
        nat = blk[perm]                      # back to natural order
        assert np.array_equal(nat, _padded(t, 256)), b
        assert not nat[t.shape[0]:].any() and not nat[:, E:].any()


@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_eval_cpu_reconstructs_per_bin(prf):
    d = _engine(prf)
    tabs = _tables()
    # repeated and unsorted bin ids; first and last row of the odd bins
    bins = [4, 0, 2, 2, 4, 1, 3, 1, 0, 3]
    rows = [4, 0, 76, 0, 0, 129, 127, 64, 0, 1]
    k1s, k2s = d.gen_batch(rows, bins)
    a = d.eval_cpu(k1s, bins)
    b = d.eval_cpu(k2s, torch.tensor(bins, dtype=torch.int64))
    assert a.shape == (len(bins), E) and a.dtype == torch.int32
    for i, (r, bn) in enumerate(zip(rows, bins)):
        own = _core.eval_fused_cpu(k1s[i].numpy(), _padded(tabs[bn], 256), prf)
        assert np.array_equal(a[i].numpy(), own[:E]), i
        if bn != 0:   # the oracle tells bins apart
            other = _core.eval_fused_cpu(k1s[i].numpy(),
                                         _padded(tabs[0], 256), prf)
            assert not np.array_equal(own, other), i
    rec = (a.to(torch.int64) - b.to(torch.int64)).to(torch.int32)
    want = torch.stack([tabs[bn][r] for r, bn in zip(rows, bins)])
    assert torch.equal(rec, want)
    # single keys through gen()
    k1, k2 = d.gen(76, 2)
    rec = (d.eval_cpu([k1], [2]).to(torch.int64)
           - d.eval_cpu([k2], [2]).to(torch.int64)).to(torch.int32)
    assert torch.equal(rec[0], tabs[2][76])


def test_host_rejections():
    d = _engine(DPF.PRF_SALSA20)
    k1s, _ = d.gen_batch([0, 1, 2], [1, 1, 2])
    # bin ids: out of range, negative, not integers, not 1-D, on the way in
    # through every entry point that takes them
    for bad, msg in [([0, 5, 1], r"\[0, 5\)"), ([0, -1, 1], r"\[0, 5\)"),
                     ([0.0, 1.0, 2.0], "integers"),
                     (torch.tensor([0.0, 1.0, 2.0]), "integers"),
                     (torch.tensor([[0, 1, 2]]), "1-D")]:
        with pytest.raises(Exception, match=msg):
            d.bind_bins(bad)
        with pytest.raises(Exception, match=msg):
            d.eval_cpu(k1s, bad)
        with pytest.raises(Exception, match=msg):
            d.gen_batch([0, 0, 0], bad)
    assert d._plan is None                     # nothing was bound
    # length mismatches
    with pytest.raises(Exception, match="bins: 2 ids for 3 keys"):
        d.eval_cpu(k1s, [1, 1])
    with pytest.raises(Exception, match="3 indices for 2 bins"):
        d.gen_batch([0, 0, 0], [1, 1])
    # k >= n_bin, bad bin
    with pytest.raises(Exception, match="rows of bin 2"):
        d.gen(77, 2)
    with pytest.raises(Exception, match="rows of bin 0"):
        d.gen_batch([0, 1], [1, 0])
    with pytest.raises(Exception, match="out of range"):
        d.gen(0, 5)
    with pytest.raises(Exception, match="out of range"):
        d.gen(0, -1)
    d.gen(76, 2)
    # launches without / with a wrong plan raise before anything else
    out = torch.zeros((3, 16), dtype=torch.int32)
    with pytest.raises(Exception, match="bind_bins"):
        d._launch_fused(k1s, out)
    with pytest.raises(Exception, match="bind_bins"):
        d.eval_gpu_into(k1s, out)
    plan = d.bind_bins([1, 1])
    assert plan.dtype == torch.int32 and plan.tolist() == [1, 1]
    with pytest.raises(Exception, match="2 slots but the batch has 3"):
        d._launch_fused(k1s, out)
    assert not out.any()


def test_eval_init_rejections():
    d = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    with pytest.raises(Exception, match="at most 16"):
        d.eval_init([_rand((8, 17), 1), _rand((8, 17), 2)])
    with pytest.raises(Exception, match="one entry size"):
        d.eval_init([_rand((8, 4), 1), _rand((8, 5), 2)])
    with pytest.raises(Exception, match="n_b >= 1"):
        d.eval_init([_rand((8, 4), 1), _rand((0, 4), 2)])
    with pytest.raises(Exception, match="at least one"):
        d.eval_init([])
    with pytest.raises(Exception):
        d.gen(0, 0)                            # no bins declared
    # paths a binned table does not serve
    d = _engine(DPF.PRF_SALSA20)
    k1s, _ = d.gen_batch([0], [1])
    with pytest.raises(NotImplementedError):
        d.eval_gpu(k1s, [1], one_hot_only=True)
    for strategy in ("two_stage", "bfs", "coop"):
        with pytest.raises(NotImplementedError):
            d.eval_gpu(k1s, [1], strategy=strategy)
    with pytest.raises(NotImplementedError):
        d.eval_init_empty(128, 4)
    with pytest.raises(NotImplementedError):
        d.table_write([0], _rand((1, E), 3))
    with pytest.raises(NotImplementedError):
        d.table_read([0])


def test_client_needs_only_bin_sizes():
    srv = _engine(DPF.PRF_CHACHA20)
    cli = BinnedDPF(prf=DPF.PRF_CHACHA20, device="cpu")
    cli.set_bin_sizes(SIZES)
    k1, k2 = cli.gen(129, 1)
    rec = (srv.eval_cpu([k1], [1]).to(torch.int64)
           - srv.eval_cpu([k2], [1]).to(torch.int64)).to(torch.int32)
    assert torch.equal(rec[0], _tables()[1][129])


# ---------------------------------------------------------------------------
# pir.serve: planner -> bin tables -> queries -> shares -> entries
# ---------------------------------------------------------------------------
N_ENTRIES, N_BINS, SERVE_E = 2000, 16, 8


@functools.lru_cache(maxsize=None)
def plan(queries_per_bin, group_size):
    rnd = random.Random(7)
    pats = [[min(N_ENTRIES - 1, int(rnd.paretovariate(1.1)) * 3 + rnd.randrange(3))
             for _ in range(24)] for _ in range(300)]
    opt = BatchPIROptimize(
        N_ENTRIES, pats, HotColdConfig(hot_fraction=0.02),
        CollocateConfig(group_size=group_size),
        PIRConfig(num_bins=N_BINS, queries_per_bin=queries_per_bin))
    table = _rand((N_ENTRIES, SERVE_E), 99)
    return opt, table, tuple(pats)


def requests(opt, pats):
    rnd = random.Random(11)
    cold = opt.cold_entries
    return [pats[0], pats[1],
            [rnd.choice(cold) for _ in range(40)],      # budget overflows
            [cold[0]], sorted(opt.hot_set)[:3]]         # one bin; no bin


def round_trip(opt, table, dpf, indices, shares):
    """One request through `shares(keys) -> [slots, width]`; checks it
    against opt.fetch and the table."""
    e = int(table.shape[1])
    k1s, k2s, meaning = serve.make_queries(opt, dpf, indices)
    slots = opt.pir.num_bins * opt.pir.queries_per_bin
    assert k1s.shape == k2s.shape == (slots, DPF.KEY_INTS)
    assert len(meaning) == slots
    got = serve.decode(opt, meaning, shares(k1s), shares(k2s), e)
    recovered, stats = opt.fetch(indices)
    assert stats["queries_total"] == slots
    assert sum(m is not None for m in meaning) == stats["queries_used"]
    assert set(got) == {i for i in recovered if i not in opt.hot_set}
    for i, row in got.items():
        assert torch.equal(row, table[i]), i
    return got


@pytest.mark.parametrize("group_size", [1, 2])
@pytest.mark.parametrize("queries_per_bin", [1, 2])
def test_serve_round_trip_cpu(queries_per_bin, group_size):
    opt, table, pats = plan(queries_per_bin, group_size)
    tables = serve.bin_tables(opt, table)
    assert len(tables) == N_BINS
    assert all(t.shape[1] == group_size * SERVE_E for t in tables)
    for b, t in enumerate(tables):
        gids = sorted(opt.bins.get(b, []))
        assert t.shape[0] == max(1, len(gids))
        for r in (0, len(gids) - 1):
            if gids:
                cat = table[opt.groups[gids[r]]].reshape(-1)
                assert torch.equal(t[r, : len(cat)], cat)
                assert not t[r, len(cat):].any()
    bins = serve.slot_bins(opt)
    assert bins == [b for b in range(N_BINS) for _ in range(queries_per_bin)]
    dpf = BinnedDPF(prf=DPF.PRF_CHACHA20, device="cpu")
    dpf.eval_init(tables)
    n_rec = 0
    for indices in requests(opt, pats):
        n_rec += len(round_trip(opt, table, dpf, indices,
                                lambda k: dpf.eval_cpu(k, bins)))
    assert n_rec > 0


def test_bin_tables_rejects_wide_groups():
    opt, _table, _ = plan(1, 2)
    with pytest.raises(Exception, match="at most 16"):
        serve.bin_tables(opt, _rand((N_ENTRIES, 9), 1))


def test_empty_bins_get_a_zero_row():
    pats = [[1, 2, 3]]
    opt = BatchPIROptimize(3, pats, pir=PIRConfig(num_bins=16))
    tables = serve.bin_tables(opt, _rand((3, 4), 5))
    assert len(tables) == 16
    empty = [b for b in range(16) if b not in opt.bins]
    assert empty
    for b in empty:
        assert tables[b].shape == (1, 4) and not tables[b].any()
