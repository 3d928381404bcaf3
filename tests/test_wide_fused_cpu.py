"""fused_words: the opt-in row width of the fused kernel, host side.

No GPU: the knob's validation, BinnedDPF admitting and refusing entry sizes
by it, the CPU round trip over wide bins, and pir.serve laying out and
decoding a collocated plan whose rows are wider than 16 words.
"""

import functools
import random

import pytest
import torch

from gpudpf import BinnedDPF, DPF
from pir import (BatchPIROptimize, CollocateConfig, HotColdConfig, PIRConfig,
                 serve)


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


def test_the_limit_is_stated_once():
    from gpudpf import _core
    assert DPF.MAX_FUSED_WORDS == _core.MAX_FUSED_WORDS == 64
    assert DPF.FUSED_WIDTHS == (16, 32, 48, 64)


def test_defaults_are_sixteen_words():
    assert DPF().fused_words == 16
    assert BinnedDPF().fused_words == 16
    assert DPF(prf=DPF.PRF_SALSA20, device="cpu").fused_words == 16


@pytest.mark.parametrize("cls", [DPF, BinnedDPF])
def test_fused_words_validation(cls):
    for ok in (16, 32, 48, 64):
        assert cls(fused_words=ok).fused_words == ok
    for bad in (0, 8, 40, 80):
        with pytest.raises(Exception, match="fused_words"):
            cls(fused_words=bad)


def test_fused_servable_follows_the_knob():
    table = _rand((200, 33), 1)
    for words, servable in [(16, False), (32, False), (48, True), (64, True)]:
        d = DPF(prf=DPF.PRF_SALSA20, device="cpu", fused_words=words)
        d.eval_init(table)
        assert d._entry_padded == 48
        assert d.fused_servable is servable, words


@pytest.mark.parametrize("e", [17, 40, 64])
def test_binned_admits_up_to_fused_words(e):
    d = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu", fused_words=64)
    d.eval_init([_rand((8, e), 1), _rand((5, e), 2)])
    assert d.table_effective_entry_size == e
    assert d._entry_padded == -(-e // 16) * 16 and d.fused_servable
    blk = d.bin_block(1)
    assert blk.shape == (128, d._entry_padded)
    nat = blk[d._perm]                       # back to natural order
    assert torch.equal(nat[:5, :e], d.tables[1])
    assert not nat[5:].any() and not nat[:, e:].any()


def test_binned_refuses_beyond_fused_words():
    d = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu", fused_words=64)
    with pytest.raises(Exception, match="at most 64"):
        d.eval_init([_rand((8, 65), 1)])
    d = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu", fused_words=32)
    with pytest.raises(Exception, match="at most 32"):
        d.eval_init([_rand((8, 33), 1)])
    d.eval_init([_rand((8, 32), 1)])


@pytest.mark.parametrize("e", [40, 64])
def test_binned_eval_cpu_round_trip_wide(e):
    sizes = [200, 1, 129]
    tabs = [_rand((n, e), 10 * e + b) for b, n in enumerate(sizes)]
    d = BinnedDPF(prf=DPF.PRF_CHACHA20, device="cpu", fused_words=64)
    d.eval_init(tabs)
    assert d._n_domain == 256
    bins = [2, 0, 1, 2, 0, 2]
    rows = [128, 199, 0, 0, 0, 64]
    k1s, k2s = d.gen_batch(rows, bins)
    a, b = d.eval_cpu(k1s, bins), d.eval_cpu(k2s, bins)
    assert a.shape == (len(bins), e) and a.dtype == torch.int32
    rec = (a.to(torch.int64) - b.to(torch.int64)).to(torch.int32)
    want = torch.stack([tabs[bn][r] for r, bn in zip(rows, bins)])
    assert torch.equal(rec, want)


# ---------------------------------------------------------------------------
# pir.serve over a collocated plan: group_size 2 of 24-word entries = 48 words
# ---------------------------------------------------------------------------
N_ENTRIES, N_BINS, SERVE_E = 2000, 16, 24


@functools.lru_cache(maxsize=None)
def wide_plan(queries_per_bin=2, group_size=2):
    rnd = random.Random(7)
    pats = [[min(N_ENTRIES - 1,
                 int(rnd.paretovariate(1.1)) * 3 + rnd.randrange(3))
             for _ in range(24)] for _ in range(300)]
    opt = BatchPIROptimize(
        N_ENTRIES, pats, HotColdConfig(hot_fraction=0.02),
        CollocateConfig(group_size=group_size),
        PIRConfig(num_bins=N_BINS, queries_per_bin=queries_per_bin))
    return opt, _rand((N_ENTRIES, SERVE_E), 99), tuple(pats)


def wide_requests(opt, pats):
    rnd = random.Random(11)
    cold = opt.cold_entries
    return [pats[0], pats[1], [rnd.choice(cold) for _ in range(40)],
            [cold[0]], sorted(opt.hot_set)[:3]]


def wide_round_trip(opt, table, dpf, indices, shares):
    """One request through `shares(keys) -> [slots, width]`, checked
    against opt.fetch and the table; returns what it recovered."""
    e = int(table.shape[1])
    k1s, k2s, meaning = serve.make_queries(opt, dpf, indices)
    slots = opt.pir.num_bins * opt.pir.queries_per_bin
    assert k1s.shape == k2s.shape == (slots, DPF.KEY_INTS)
    got = serve.decode(opt, meaning, shares(k1s), shares(k2s), e)
    recovered, stats = opt.fetch(indices)
    assert stats["queries_total"] == slots
    assert sum(m is not None for m in meaning) == stats["queries_used"]
    assert set(got) == {i for i in recovered if i not in opt.hot_set}
    for i, row in got.items():
        assert torch.equal(row, table[i]), i
    return got


def test_bin_tables_width_limit():
    opt, table, _pats = wide_plan()
    with pytest.raises(Exception, match="at most 16"):
        serve.bin_tables(opt, table)
    with pytest.raises(Exception, match="at most 32"):
        serve.bin_tables(opt, table, max_words=32)
    tables = serve.bin_tables(opt, table, max_words=64)
    assert len(tables) == N_BINS
    assert all(t.shape[1] == 48 for t in tables)
    assert torch.equal(serve.bin_tables(opt, table, max_words=48)[3],
                       tables[3])
    for b, t in enumerate(tables):
        gids = sorted(opt.bins.get(b, []))
        assert t.shape[0] == max(1, len(gids))
        if gids:
            cat = table[opt.groups[gids[-1]]].reshape(-1)
            assert torch.equal(t[-1, : len(cat)], cat)
            assert not t[-1, len(cat):].any()


def test_serve_round_trip_cpu_wide():
    opt, table, pats = wide_plan()
    dpf = BinnedDPF(prf=DPF.PRF_CHACHA20, device="cpu", fused_words=64)
    dpf.eval_init(serve.bin_tables(opt, table, max_words=64))
    assert dpf._entry_padded == 48
    bins = serve.slot_bins(opt)
    n_rec = sum(
        len(wide_round_trip(opt, table, dpf, idx,
                            lambda keys: dpf.eval_cpu(keys, bins)))
        for idx in wide_requests(opt, pats))
    assert n_rec > 0
