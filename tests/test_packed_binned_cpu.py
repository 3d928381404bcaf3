"""gpudpf.PackedBinnedDPF on the host: domain, layout, CPU reference, the
launcher's argument checks, the units query, refusals and the pir.serve round
trip.  No GPU needed; every comparison is exact.

A packed binned engine is a BinnedDPF whose bin domain starts at 512, whose
blocks are in packed_perm order and whose keys carry lane log 2; index idx of
a bin is word idx >> D of tree node idx & (2^D - 1), D = log2(domain) - 2.
"""

import functools

import numpy as np
import pytest
import torch

import packed_binned_oracle as pbo
import packed_oracle as po
import sparse_oracle as so
from gpudpf import BinnedDPF, DPF, PackedBinnedDPF, PackedDPF, _core
from pir import serve

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}
SIZES = [1, 513, 5000]          # domain 8192, tree depth 11
DOMAIN, D, ZLOG = 8192, 11, 8
E = 5


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-(2**31), 2**31, shape, dtype=torch.int64,
                         generator=g).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _tables():
    return tuple(_rand((n, E), 700 + b) for b, n in enumerate(SIZES))


def _engine(prf):
    d = PackedBinnedDPF(prf=prf, device="cpu")
    d.eval_init(list(_tables()))
    return d


def _padded(t, n, words=16):
    p = np.zeros((n, words), dtype=np.int32)
    p[: t.shape[0], : t.shape[1]] = t.numpy()
    return p


def _edge_rows(size):
    """0, the bin's last row, and both sides of every lane boundary of the
    domain that lies inside the bin."""
    q = DOMAIN // 4
    rows = {0, size - 1}
    for k in (1, 2, 3):
        rows |= {r for r in (k * q - 1, k * q) if r < size}
    return sorted(rows)


def test_domain_and_header():
    d = _engine(DPF.PRF_SALSA20)
    assert d.num_bins == 3 and d.bin_sizes == SIZES
    assert (d._n_domain, d._depth, d._zlog) == (DOMAIN, D, ZLOG)
    assert d._n_domain == PackedDPF._domain(max(SIZES))
    assert d._zlog == _core.zlog_for_depth(D)
    assert d._entry_padded == 16 and d.table_effective_entry_size == E
    assert d.LANE_LOG == 2
    k1, k2 = d.gen(4999, 2)
    assert int(k1[0]) == D and int(k1[1]) == 2 and int(k2[1]) == 2
    k1s, _ = d.gen_batch([0, 512], [0, 1])
    assert k1s.shape == (2, DPF.KEY_INTS) and bool((k1s[:, 1] == 2).all())
    # a client that knows only the sizes gets the same domain
    cli = PackedBinnedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    cli.set_bin_sizes([1, 2, 3])
    assert cli._n_domain == 512
    assert "PackedBinnedDPF(bins=3, bin_domain=8192" in repr(d)


@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_eval_cpu_reconstructs_across_lane_boundaries_and_bin_ends(prf):
    d = _engine(prf)
    tabs = _tables()
    rows, bins = [], []
    for b, size in enumerate(SIZES):
        er = _edge_rows(size)
        rows += er
        bins += [b] * len(er)
    # bin 2 (5000 rows) crosses two lane boundaries of the 8192 domain
    # (lanes are 2048 indices) and ends inside lane 2; bins 0 and 1 end
    # inside lane 0
    assert [r for r, b in zip(rows, bins) if b == 2] == \
        [0, 2047, 2048, 4095, 4096, 4999]
    assert [r for r, b in zip(rows, bins) if b == 1] == [0, 512]
    k1s, k2s = d.gen_batch(rows, bins)
    a = d.eval_cpu(k1s, bins)
    b2 = d.eval_cpu(k2s, torch.tensor(bins, dtype=torch.int64))
    assert a.shape == (len(bins), E) and a.dtype == torch.int32
    for i, bn in enumerate(bins):
        own = _core.eval_fused_cpu(k1s[i].numpy(), _padded(tabs[bn], DOMAIN),
                                   prf)
        assert np.array_equal(a[i].numpy(), own[:E]), i
    rec = so.reconstruct(a.numpy(), b2.numpy())
    want = np.stack([tabs[bn][r].numpy() for r, bn in zip(rows, bins)])
    assert np.array_equal(rec, want)
    # past each bin's end: refused, although the domain has the index
    for b, size in enumerate(SIZES):
        with pytest.raises(Exception, match="rows of bin %d" % b):
            d.gen(size, b)
        with pytest.raises(Exception, match="rows of bin %d" % b):
            d.gen_batch([size], [b])


def test_bin_block_is_the_packed_row_formula():
    d = _engine(DPF.PRF_SALSA20)
    perm = np.array([po.packed_perm(i, D, ZLOG) for i in range(DOMAIN)])
    assert sorted(perm.tolist()) == list(range(DOMAIN))
    assert np.array_equal(perm, _core.packed_perm_table(DOMAIN, ZLOG))
    for b, t in enumerate(_tables()):
        blk = d.bin_block(b).numpy()
        assert blk.shape == (DOMAIN, 16) and blk.dtype == np.int32
        want = np.zeros((DOMAIN, 16), dtype=np.int32)
        want[perm[: t.shape[0]], :E] = t.numpy()
        assert np.array_equal(blk, want), b
        assert np.array_equal(blk[perm], _padded(t, DOMAIN)), b


def test_plain_bin_block_is_still_leaf_perm():
    sizes = [1, 130, 77]
    tabs = [_rand((n, E), 40 + b) for b, n in enumerate(sizes)]
    d = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    d.eval_init(tabs)
    assert (d._n_domain, d._depth, d.LANE_LOG) == (256, 8, 0)
    perm = _core.leaf_perm_table(256, d._zlog)
    assert np.array_equal(d._perm.numpy(), perm)
    for b, t in enumerate(tabs):
        want = np.zeros((256, 16), dtype=np.int32)
        want[perm[: t.shape[0]], :E] = t.numpy()
        assert np.array_equal(d.bin_block(b).numpy(), want), b


@pytest.mark.parametrize("queries_per_bin", [1, 2])
def test_serve_round_trip_cpu_packed(queries_per_bin):
    from test_binned_cpu import plan, requests, round_trip

    opt, table, pats = plan(queries_per_bin, 2)
    tables = serve.bin_tables(opt, table, max_words=64)
    bins = serve.slot_bins(opt)
    dpf = PackedBinnedDPF(prf=DPF.PRF_CHACHA20, device="cpu", fused_words=64)
    dpf.eval_init(tables)
    assert dpf._n_domain == 512 and dpf._depth == 7
    n_rec = 0
    for indices in requests(opt, pats):
        n_rec += len(round_trip(opt, table, dpf, indices,
                                lambda k: dpf.eval_cpu(k, bins)))
    assert n_rec > 0
    k1s, _k2s, _m = serve.make_queries(opt, dpf, pats[0])
    assert bool((k1s[:, 1] == 2).all())


def test_engines_refuse_each_others_keys():
    sizes = [600, 513]
    tabs = [_rand((n, E), 80 + b) for b, n in enumerate(sizes)]
    pb = PackedBinnedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    pb.eval_init(tabs)
    b = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    b.eval_init(tabs)
    assert pb._n_domain == b._n_domain == 1024
    pk, _ = pb.gen(3, 1)
    k, _ = b.gen(3, 1)
    assert int(pk[1]) == 2 and int(k[1]) == 0
    with pytest.raises(Exception, match="packed keys"):
        pb.eval_cpu([k], [1])
    with pytest.raises(Exception, match="plain keys"):
        b.eval_cpu([pk], [1])
    with pytest.raises(Exception, match="mixed"):
        pb.eval_cpu([pk, k], [1, 1])
    with pytest.raises(Exception, match="mixed"):
        b.eval_cpu([k, pk], [1, 1])
    with pytest.raises(Exception, match="packed keys"):
        pb._keys_tensor([k])
    # what a binned table does not serve, packed or not
    with pytest.raises(NotImplementedError):
        pb.eval_gpu([pk], [1], one_hot_only=True)
    with pytest.raises(NotImplementedError):
        pb.eval_gpu([pk], [1], strategy="two_stage")
    with pytest.raises(NotImplementedError):
        pb.eval_init_empty(512, 4)
    with pytest.raises(NotImplementedError):
        pb.table_write([0], _rand((1, E), 3))
    with pytest.raises(Exception, match="at most 16"):
        pb.eval_init([_rand((8, 17), 1)])
    wide = PackedBinnedDPF(prf=DPF.PRF_SALSA20, device="cpu", fused_words=48)
    wide.eval_init([_rand((8, 33), 1)])
    assert wide._entry_padded == 48 and wide.fused_servable
    with pytest.raises(Exception, match="at most 48"):
        wide.eval_init([_rand((8, 49), 1)])
    with pytest.raises(Exception, match="fused_words"):
        PackedBinnedDPF(fused_words=80)
    # the unbinned packed engine keeps its refusal
    with pytest.raises(Exception, match="at most 16 words"):
        PackedDPF(fused_words=32)


# ---------------------------------------------------------------------------
# Launcher argument checks: null pointers, so nothing may reach a kernel
# ---------------------------------------------------------------------------
GOOD = dict(n=4 << 12, depth=12, zlog=8, num_bins=2, bins=64, out=0,
            entry_words=16, scratch=0, scratch_bytes=0)
# sibling-stack scratch of batch 1 at D = 16: slog 6, one global level
NEED_16 = (1 << 6) * 1 * 256 * 16
BAD_LAUNCHES = [
    (dict(entry_words=17), "entry_words"),
    (dict(entry_words=80), "entry_words"),
    (dict(n=4 << 6, depth=6, zlog=5), "depth"),
    (dict(n=4 << 33, depth=33), "depth"),
    (dict(n=1 << 12), "4 << depth"),              # the plain n
    (dict(n=(4 << 12) + 4), "4 << depth"),
    (dict(zlog=5), "zlog"),
    (dict(zlog=12), "zlog"),
    (dict(num_bins=0), "num_bins"),
    (dict(num_bins=-1), "num_bins"),
    (dict(num_bins=1 << 50), "overflows"),
    (dict(num_bins=1 << 46, entry_words=64), "overflows"),
    (dict(bins=0), "bins"),
    (dict(out=8), "16-byte aligned"),
    (dict(n=4 << 16, depth=16, scratch=64, scratch_bytes=NEED_16 - 1),
     "scratch"),
]


@pytest.mark.parametrize("args,msg", BAD_LAUNCHES)
def test_packed_binned_launcher_checks_arguments(args, msg):
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    assert _hip.eval_scratch_bytes(1, 16, 8) == NEED_16
    kw = dict(GOOD)
    kw.update(args)
    with pytest.raises(ValueError, match=msg):
        _hip.eval_fused_packed_binned(keys=0, table=0, aes_tabs=0, batch=1,
                                      prf=DPF.PRF_DUMMY, stream=0, **kw)


def test_packed_units_per_wg_query(monkeypatch):
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    aes = DPF.PRF_AES128
    monkeypatch.delenv("GPUDPF_AES_UNITS", raising=False)
    for words in (16, 32, 48, 64):
        for prf in PRFS[:3]:
            assert _hip.eval_units_per_wg_packed(prf, 1000, words) == 1
        for n_units in (1, 7, 1000, 2048):
            assert _hip.eval_units_per_wg_packed(aes, n_units, words) \
                == (3 if words == 16 else 2)
    for forced in (1, 2, 3, 4):
        monkeypatch.setenv("GPUDPF_AES_UNITS", str(forced))
        assert _hip.eval_units_per_wg_packed(aes, 1000, 16) == min(forced, 3)
        for words in (32, 48, 64):
            assert _hip.eval_units_per_wg_packed(aes, 1000, words) \
                == min(forced, 2)
        assert _hip.eval_units_per_wg_packed(DPF.PRF_CHACHA20, 1000, 64) == 1
    for words in (17, 0, 80):
        with pytest.raises(ValueError, match="entry_words"):
            _hip.eval_units_per_wg_packed(aes, 1000, words)
    assert _hip.eval_units_per_wg_packed(prf=aes, n_units=5,
                                         entry_words=32) == 2
    # the older query still speaks for 16-word packed launches only
    with pytest.raises(ValueError, match="lanes"):
        _hip.eval_units_per_wg(aes, 1000, 32, lanes=4)
    assert _hip.eval_units_per_wg(aes, 1000, 16, lanes=4) == 3


# ---------------------------------------------------------------------------
# The large-offset shape of test_gpu_packed_binned.py, by arithmetic
# ---------------------------------------------------------------------------
def test_large_offset_rows_straddle_every_boundary():
    n, words, bins = pbo.LARGE_N, pbo.LARGE_WORDS, pbo.LARGE_BINS
    assert n == 1 << 26 and (bins * n * words * 4) == 20 << 30
    assert 4 * n * words == 1 << 32          # bin 4 starts at element 2^32
    assert 2 * n * words == 1 << 31 and n * words * 4 == 1 << 32
    assert so.crossed(bins * n, words) == pbo.LARGE_CROSSED
    flat = pbo.large_flat_rows()
    rep = so.straddle_report(flat, bins * n, words, po.other_leaf)
    assert sorted(rep) == sorted(pbo.LARGE_CROSSED)
    for name, r in rep.items():
        assert all(r.values()), (name, r)
    for b in range(bins):       # every block holds its first and last row
        assert b * n in flat and (b + 1) * n - 1 in flat
    sts = pbo.large_bin_tables(flat)
    assert sum(len(st.prow) for st in sts) == len(flat)
    zlog = so.zlog_of(pbo.LARGE_D)
    for st in sts:
        assert st.prow[0] == 0 and st.prow[-1] == n - 1
        for r, i in zip(st.prow[:8], st.nat[:8]):
            assert po.packed_perm(int(i), pbo.LARGE_D, zlog) == r
