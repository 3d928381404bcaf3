"""Packed DPF keys on the CPU: scheme, wire format, row order and refusals.

A packed key over n = 2^d rows has tree depth D = d - 2; index idx is word
idx >> D of the last level's 128-bit output at node idx & (2^D - 1).  All
comparisons are exact integers.
"""

import functools

import numpy as np
import pytest
import torch

import packed_oracle as po
import sparse_oracle as so
from gpudpf import DPF, BinnedDPF, PackedDPF, _core

try:
    from gpudpf import _hip
except ImportError:  # no HIP runtime on this machine
    _hip = None

PRFS = [DPF.PRF_DUMMY, DPF.PRF_SALSA20, DPF.PRF_CHACHA20, DPF.PRF_AES128]
PRF_IDS = {DPF.PRF_DUMMY: "dummy", DPF.PRF_SALSA20: "salsa",
           DPF.PRF_CHACHA20: "chacha", DPF.PRF_AES128: "aes"}


def _alphas(n):
    """0, n-1, one value inside each lane, both sides of every lane
    boundary."""
    q = n // 4
    inner = [k * q + 37 + 11 * k for k in range(4)]
    edges = [k * q - 1 for k in range(1, 4)] + [k * q for k in range(1, 4)]
    out = sorted(set([0, n - 1] + inner + edges))
    assert {a // q for a in inner} == {0, 1, 2, 3}
    return out


@functools.lru_cache(maxsize=None)
def _table(n, e=16):
    g = torch.Generator().manual_seed(7000 + n + e)
    return torch.randint(-(2**31), 2**31, (n, e), dtype=torch.int64,
                         generator=g).to(torch.int32).numpy()


def _gen(alpha, n, prf):
    return _core.gen(alpha, n, b"packed-%d-%d-%d" % (alpha, n, prf), prf,
                     packed=True)


# ---------------------------------------------------------------------------
# Full domain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 2048])
@pytest.mark.parametrize("prf", PRFS, ids=PRF_IDS.get)
def test_packed_full_domain(prf, n):
    table = _table(n)
    t64 = table.astype(np.int64)
    for alpha in _alphas(n):
        k1, k2 = _gen(alpha, n, prf)
        e1, e2 = _core.expand(k1, prf), _core.expand(k2, prf)
        assert e1.shape == (n,)
        one_hot = np.zeros(n, dtype=np.int32)
        one_hot[alpha] = 1
        assert np.array_equal(so.reconstruct(e1, e2), one_hot), alpha
        for k, e in ((k1, e1), (k2, e2)):
            pts = so.point_shares(k, range(n), prf).astype(np.uint32)
            assert np.array_equal(pts.view(np.int32), e), alpha
            fused = _core.eval_fused_cpu(k, table, prf)
            want = (e.astype(np.int64) @ t64).astype(np.int32)
            assert np.array_equal(fused, want), alpha
        # the threaded batch expansion takes no subkeys of a packed key
        eb = _core.expand_batch([k1, k2], prf, 8)
        assert np.array_equal(eb[0], e1) and np.array_equal(eb[1], e2)


# ---------------------------------------------------------------------------
# Header and wire format
# ---------------------------------------------------------------------------
def _header(k):
    n = (int(k[521]) << 32) | (int(k[520]) & 0xFFFFFFFF)
    return int(k[0]), int(k[1]), n


@pytest.mark.parametrize("d", [9, 11, 20, 32])
def test_packed_header(d):
    n = 1 << d
    for k in _core.gen(n - 3, n, b"hdr", DPF.PRF_DUMMY, packed=True):
        assert _header(k) == (d - 2, 2, n)
        assert k.shape == (524,) and k.dtype == np.int32
    for k in _core.gen(n - 3, n, b"hdr", DPF.PRF_DUMMY):
        assert _header(k) == (d, 0, n)


def test_packed_needs_domain_512():
    with pytest.raises(ValueError, match="512"):
        _core.gen(3, 256, b"x", DPF.PRF_DUMMY, packed=True)


# _core.gen(77, 4096, b"pin-seed", PRF_AES128) of the commit before packed
# keys existed: ints 0..7 and 516..523 of both keys (header, the first
# correction word, root seed, n) and the sum of all 524 ints mod 2^32.
PARENT_PIN = None  # filled in below


def _pin(keys):
    return [(k[:8].tolist(), k[516:].tolist(),
             int(k.astype(np.int64).sum() & 0xFFFFFFFF)) for k in keys]


def test_default_mode_keys_are_the_plain_keys():
    """The keyword's default is today's scheme, byte for byte: with and
    without it, and against values recorded before the keyword existed."""
    for prf in PRFS:
        a = _core.gen(77, 4096, b"pin-seed", prf)
        b = _core.gen(77, 4096, b"pin-seed", prf, packed=False)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        c = _core.gen(77, 4096, b"pin-seed", prf, packed=True)
        assert a[0].tobytes() != c[0].tobytes()
    al = np.array([5, 4000], dtype=np.int64)
    a = _core.gen_batch(al, 4096, b"pin-seed", DPF.PRF_SALSA20)
    b = _core.gen_batch(al, 4096, b"pin-seed", DPF.PRF_SALSA20, packed=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert _pin(_core.gen(77, 4096, b"pin-seed", DPF.PRF_AES128)) \
        == PARENT_PIN


def test_packed_compact_round_trip():
    k1, _ = _gen(1234, 4096, DPF.PRF_CHACHA20)
    kt = torch.from_numpy(k1)
    c = DPF.key_compact(kt)
    assert c.numel() == (3 + 4 * 10) * 4  # tree depth 10
    assert int(c[1]) == 2
    assert torch.equal(DPF.key_expand(c), kt)
    bad = c.clone()
    bad[1] = 1
    with pytest.raises(ValueError, match="lane log"):
        DPF.key_expand(bad)
    bad = c.clone()
    bad[-4] = 2048  # n != 2^(D+2)
    with pytest.raises(ValueError, match="n != 2"):
        DPF.key_expand(bad)


def test_packed_deserialize_refuses_bad_headers():
    k1, _ = _gen(9, 2048, DPF.PRF_DUMMY)
    assert _core.expand(k1, DPF.PRF_DUMMY).shape == (2048,)
    for n_bad in (512, 1024, 4096):  # n != 2^(D+2) = 2048
        bad = k1.copy()
        bad[520] = n_bad
        with pytest.raises(ValueError, match="n != 2"):
            _core.expand(bad, DPF.PRF_DUMMY)
    for lanes in (1, 3, 4, -1):
        bad = k1.copy()
        bad[1] = lanes
        with pytest.raises(ValueError, match="lane log"):
            _core.expand(bad, DPF.PRF_DUMMY)
    plain = k1.copy()
    plain[1] = 0  # then n must be 2^D
    with pytest.raises(ValueError, match="n != 2"):
        _core.expand(plain, DPF.PRF_DUMMY)


def test_packed_keys_have_no_subkeys_and_no_u128_shares():
    k1, _ = _gen(9, 2048, DPF.PRF_DUMMY)
    with pytest.raises(ValueError, match="packed"):
        _core.shard_subkey(k1, DPF.PRF_DUMMY, 0, 2)
    with pytest.raises(ValueError, match="packed"):
        _core.shard_subkey_batch(k1[None], DPF.PRF_DUMMY, 0, 2)
    with pytest.raises(ValueError, match="packed"):
        _core.eval_point128(k1, 5, DPF.PRF_DUMMY)


# ---------------------------------------------------------------------------
# Row order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", range(7, 15))
def test_packed_perm_is_the_row_formula(D):
    n = 4 << D
    zlog = _core.zlog_for_depth(D)
    assert zlog == so.zlog_of(D)
    perm = _core.packed_perm_table(n, zlog)
    assert perm.shape == (n,)
    assert np.array_equal(np.sort(perm), np.arange(n))  # a bijection
    step = 1 if D <= 10 else 37
    idx = np.arange(0, n, step, dtype=np.int64)
    want = np.array([po.packed_perm(int(i), D, zlog) for i in idx])
    assert np.array_equal(perm[idx], want)
    assert np.array_equal(_core.packed_perm_rows(idx, n, zlog), want)
    assert all(po.packed_perm_inv(int(r), D, zlog) == int(i)
               for i, r in zip(idx[:4096], want[:4096]))
    # a thread's 8 rows: b << 2 | lane over the two leaves and four lanes
    node = 5 % (1 << D)
    rows = [int(perm[(node | (b << (D - 1))) + lane * (1 << D)])
            for b in range(2) for lane in range(4)]
    assert rows == list(range(rows[0], rows[0] + 8)) and rows[0] % 8 == 0
    with pytest.raises(IndexError):
        _core.packed_perm_rows(np.array([n]), n, zlog)


def test_packed_perm_is_leaf_perm_times_four_plus_lane():
    D, zlog = 12, 8
    leaf = _core.leaf_perm_table(1 << D, zlog)
    perm = _core.packed_perm_table(4 << D, zlog).reshape(4, 1 << D)
    for lane in range(4):
        assert np.array_equal(perm[lane], leaf * 4 + lane)


def test_large_offset_rows_straddle_every_boundary():
    """The S of the packed large-offset GPU test holds rows below, across
    and above bytes 2^31 and 2^32 of the 8 GiB table.  The table is 2^31
    elements, so it ENDS at element 2^31 (sparse_oracle counts a boundary as
    crossed only with an element at or past it): there S holds the last
    leaf pair, whose final element has the largest 31-bit offset, and no
    row can lie above."""
    n = 4 << po.LARGE_D
    assert n * po.LARGE_WORDS * 4 == 8 << 30
    assert n * po.LARGE_WORDS == so.BOUNDARY["elem 2^31"]
    assert so.crossed(n, po.LARGE_WORDS) == po.LARGE_CROSSED
    rows = po.large_rows()
    assert len(rows) < 200
    rep = so.straddle_report(rows, n, po.LARGE_WORDS, po.other_leaf)
    assert sorted(rep) == sorted(po.LARGE_CROSSED)
    for name, r in rep.items():
        assert all(r.values()), (name, r)
    assert n - 1 in rows and po.other_leaf(n - 1) in rows
    # and S maps to distinct natural indices in all four lanes
    zlog = so.zlog_of(po.LARGE_D)
    nat = [po.packed_perm_inv(r, po.LARGE_D, zlog) for r in rows]
    assert len(set(nat)) == len(rows)
    assert {a >> po.LARGE_D for a in nat} == {0, 1, 2, 3}
    back = _core.packed_perm_rows(np.array(nat, dtype=np.int64), n, zlog)
    assert back.tolist() == rows


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def test_packed_api_refusals():
    n = 2048
    pd = PackedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    d = DPF(prf=DPF.PRF_SALSA20, device="cpu")
    pk, _ = pd.gen(3, n)
    k, _ = d.gen(3, n)
    assert int(pk[1]) == 2 and int(k[1]) == 0
    assert pd.eval_cpu([pk], one_hot_only=True).shape == (1, n)
    with pytest.raises(Exception, match="plain keys"):
        d.eval_cpu([pk], one_hot_only=True)
    with pytest.raises(Exception, match="packed keys"):
        pd.eval_cpu([k], one_hot_only=True)
    with pytest.raises(Exception, match="mixed"):
        pd.eval_cpu([pk, k], one_hot_only=True)
    with pytest.raises(Exception, match="mixed"):
        d.eval_cpu([k, pk], one_hot_only=True)
    b = BinnedDPF(prf=DPF.PRF_SALSA20, device="cpu")
    with pytest.raises(Exception, match="plain keys"):
        b._keys_tensor([pk])
    with pytest.raises(Exception, match="at most 16 words"):
        PackedDPF(fused_words=32)
    pd.eval_init(torch.from_numpy(_table(n)))
    for strategy in ("bfs", "coop"):
        with pytest.raises(NotImplementedError, match="fused"):
            pd.eval_gpu([pk], strategy=strategy)


def test_packed_gen_batch_and_domain():
    pd = PackedDPF(prf=DPF.PRF_CHACHA20, device="cpu")
    assert [pd._domain(n) for n in (1, 512, 513, 5000)] \
        == [512, 512, 1024, 8192]
    idx = [0, 700, 1023, 256]
    k1s, k2s = pd.gen_batch(idx, 1024)
    assert k1s.shape == (4, 524) and bool((k1s[:, 1] == 2).all())
    rec = (pd.eval_cpu(k1s, one_hot_only=True)
           - pd.eval_cpu(k2s, one_hot_only=True)).numpy()
    want = np.zeros((4, 1024), dtype=np.int32)
    want[np.arange(4), idx] = 1
    assert np.array_equal(rec, want)
    pd.eval_init(torch.from_numpy(_table(1024)))
    assert (pd._depth, pd._n_domain, pd._zlog) == (8, 1024, 7)


@pytest.mark.parametrize("n", [100, 513, 1000])
def test_packed_non_power_of_two_tables(n):
    table = torch.from_numpy(_table(n, 5))
    pd = PackedDPF(prf=DPF.PRF_AES128, device="cpu")
    pd.eval_init(table)
    assert pd._n_domain == max(512, 1 << (n - 1).bit_length())
    for alpha in (n - 1, 0):
        k1, k2 = pd.gen(alpha, n)
        rec = so.reconstruct(pd.eval_cpu([k1]).numpy(),
                             pd.eval_cpu([k2]).numpy())
        assert np.array_equal(rec[0], table[alpha].numpy()), alpha


# ---------------------------------------------------------------------------
# Launcher argument checks: null pointers, so nothing may reach a kernel
# ---------------------------------------------------------------------------
BAD_LAUNCHES = [
    (dict(n=1 << 12, depth=12, zlog=8), "4 << depth"),    # the plain n
    (dict(n=(4 << 12) + 4, depth=12, zlog=8), "4 << depth"),
    (dict(n=4 << 6, depth=6, zlog=5), "depth"),
    (dict(n=4 << 33, depth=33, zlog=8), "depth"),
    (dict(n=4 << 12, depth=12, zlog=5), "zlog"),
    (dict(n=4 << 12, depth=12, zlog=12), "zlog"),
    (dict(n=4 << 7, depth=7, zlog=7), "zlog"),
]


@pytest.mark.parametrize("args,msg", BAD_LAUNCHES)
@pytest.mark.parametrize("fused", [True, False])
def test_packed_launchers_check_arguments(fused, args, msg):
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    with pytest.raises(ValueError, match=msg):
        if fused:
            _hip.eval_fused_packed(keys=0, table=0, out=0, aes_tabs=0,
                                   batch=1, prf=DPF.PRF_DUMMY, stream=0,
                                   **args)
        else:
            _hip.eval_expand_packed(keys=0, out=0, aes_tabs=0, batch=1,
                                    prf=DPF.PRF_DUMMY, stream=0, **args)


def test_packed_units_per_wg_host_arithmetic():
    if _hip is None:
        pytest.skip("gpudpf._hip cannot be imported")
    for prf in PRFS[:3]:
        assert _hip.eval_units_per_wg(prf, 1000, 16, lanes=4) == 1
    with pytest.raises(ValueError, match="lanes"):
        _hip.eval_units_per_wg(DPF.PRF_AES128, 1000, 32, lanes=4)
    with pytest.raises(ValueError, match="lanes"):
        _hip.eval_units_per_wg(DPF.PRF_AES128, 1000, 16, lanes=2)


PARENT_PIN = [
    ([12, 0, 0, 0, -510392794, 2111874008, 1205109661, -1658722951],
     [-317560138, 2101379310, 30431050, -757109999, 4096, 0, 0, 0],
     1826149056),
    ([12, 0, 0, 0, -510392794, 2111874008, 1205109661, -1658722951],
     [-127493527, -799991813, -2999776, 1756668114, 4096, 0, 0, 0],
     1595191831),
]
