"""Packed DPF keys: four 32-bit leaves per seed, a quarter of the PRF calls.

A plain key's leaf keeps the low word of a 128-bit PRF block and drops the
other 96 bits.  A packed key stops the GGM tree two levels early, at depth
D = log2(n) - 2, and reads the last level's block as four independent u32
leaves (lanes): index idx is word idx >> D of node idx & (2^D - 1).  A key
then costs n/2 - 2 PRF blocks instead of 2n - 2, for the same table and the
same shares' width (DPF.md, "Packed keys").

Packed keys are not interoperable with the reference's (int 1 of a key is 2
where plain keys have 0) and neither engine accepts the other's keys.  The
table lives in the packed row order (a node's four lanes are adjacent rows,
csrc/core/dpf_core.h) and every launch goes to the packed kernels.  What
DPF serves with one table PackedDPF serves the same way:

    d = PackedDPF(prf=DPF.PRF_AES128)
    k1, k2 = d.gen(k, n)          # any n >= 1; domains start at 512
    d.eval_init(table)            # [n, e] int32
    shares = d.eval_gpu([k1])     # fused for e <= 16, two-stage above

including eval_init_empty / table_write / table_read, one_hot_only,
eval_gpu_into, eval_cpu and the Graphed / Pipelined / TwoStage servers.

PackedBinnedDPF is BinnedDPF with packed keys: batch-PIR bins of rows of 16,
32, 48 or 64 words, one fused launch, behind the same servers and pir.serve:

    d = PackedBinnedDPF(prf=DPF.PRF_AES128, fused_words=64)
    d.eval_init(tables)                  # list of [n_b, e] int32, e <= 64
    k1s, k2s = d.gen_batch(rows, bins)   # packed keys of the bin domain
    d.bind_bins(bins)
    shares = GraphedServer(d, batch=len(bins)).eval(k1s)

With one bin it serves a plain table, which is the way to packed fused rows
wider than 16 words.

Not built, and refused: sharding (ShardedDPF), the HTTP server, the "bfs" and
"coop" strategies, and PackedDPF itself with fused rows wider than 16 words
(they take the two-stage path, or a one-bin PackedBinnedDPF).  BinnedDPF
still refuses packed keys and PackedBinnedDPF plain ones.
"""

import torch

from gpudpf import _core
from gpudpf.binned import BinnedDPF
from gpudpf.dpf import DPF, _check_arg, _hip


class _PackedLayout(object):
    """What makes an engine a packed one, in front of DPF in the bases of
    PackedDPF and PackedBinnedDPF: keys with lane log 2 (gen, gen_batch and
    _keys_tensor read LANE_LOG, _setup_domain takes it off the depth),
    domains from 512, rows in packed_perm order."""
    LANE_LOG = _core.PACKED_LANE_LOG        # 2: four lanes
    MIN_DOMAIN = _core.PACKED_MIN_DOMAIN    # 512: tree depth >= 7

    @staticmethod
    def _domain(n):
        """Next power of two >= 512: the tree over the n / 4 nodes keeps
        the depth >= 7 the kernels need."""
        d = _PackedLayout.MIN_DOMAIN
        while d < n:
            d <<= 1
        return d

    # ------------------------------------------------------------------
    # Row order: packed_perm, over the whole domain
    # ------------------------------------------------------------------
    def _perm_rows(self, indices):
        return torch.from_numpy(
            _core.packed_perm_rows(indices.to(torch.int64).cpu().numpy(),
                                   self._n_domain, self._zlog))

    def _perm_table(self):
        return torch.from_numpy(
            _core.packed_perm_table(self._n_domain, self._zlog))


class PackedDPF(_PackedLayout, DPF):
    def __init__(self, prf=None, device=None, fused_words=16):
        if fused_words != self.ENTRY_SIZE:
            raise Exception(
                "the packed fused kernel serves rows of at most %d words "
                "(got fused_words=%r); wider tables take the two-stage path, "
                "or a one-bin PackedBinnedDPF(fused_words=%r)"
                % (self.ENTRY_SIZE, fused_words, fused_words))
        super().__init__(prf=prf, device=device, fused_words=fused_words)

    # ------------------------------------------------------------------
    # Launches: _depth is the tree depth D, _n_domain the 4 << D rows
    # ------------------------------------------------------------------
    def _launch_fused(self, keys_gpu, out_gpu, scratch=None):
        b = len(keys_gpu)
        ew = self._fused_entry_words()
        stream, sptr, sbytes = self._launch_args(
            keys_gpu, (b, self.KEY_INTS), out_gpu, (b, ew), scratch)
        _hip.eval_fused_packed(
            keys_gpu.data_ptr(), self._table_gpu.data_ptr(),
            out_gpu.data_ptr(), self._aes_ptr, b, self._n_domain,
            self._depth, self._zlog, self.prf_method, stream, sptr, sbytes)

    def _launch_expand(self, keys_gpu, shares_gpu, scratch=None):
        """shares_gpu [b,n] = one-hot shares, rows in packed_perm order."""
        b = len(keys_gpu)
        stream, sptr, sbytes = self._launch_args(
            keys_gpu, (b, self.KEY_INTS), shares_gpu, (b, self._n_domain),
            scratch)
        _hip.eval_expand_packed(
            keys_gpu.data_ptr(), shares_gpu.data_ptr(), self._aes_ptr, b,
            self._n_domain, self._depth, self._zlog, self.prf_method, stream,
            sptr, sbytes)

    def _launch_bfs(self, keys_gpu, shares_gpu):
        raise NotImplementedError("packed keys have no bfs strategy")

    def _launch_coop(self, key_row, out_row, fused):
        raise NotImplementedError("packed keys have no coop strategy")

    def eval_gpu(self, keys, one_hot_only=False, strategy="fused",
                 out_device=False):
        """As DPF.eval_gpu, with the strategies "fused" and "two_stage"."""
        if strategy in ("bfs", "coop"):
            raise NotImplementedError(
                "packed keys are served by the 'fused' and 'two_stage' "
                "strategies only (got %r)" % (strategy,))
        return super().eval_gpu(keys, one_hot_only=one_hot_only,
                                strategy=strategy, out_device=out_device)

    def __repr__(self):
        return "Packed" + super().__repr__()


class PackedBinnedDPF(_PackedLayout, BinnedDPF):
    """BinnedDPF served with packed keys: batch-PIR bins, a quarter of the
    PRF blocks per key, rows of 16, 32, 48 or 64 words (fused_words), one
    fused launch (the LANES = 4 binned kernel, csrc/hip/dpf_eval.hip).

    Everything is BinnedDPF's (set_bin_sizes, gen, gen_batch, bind_bins,
    bin_block, eval_gpu, eval_cpu, eval_gpu_into, the servers, pir.serve, the
    refusals of one-hot output, two-stage and ingest) except that the bin
    domain is PackedDPF._domain(largest bin) >= 512, every block is in
    packed_perm order, _depth is the tree depth D = log2(domain) - 2 and
    plain keys are refused.  With one bin it serves an unbinned table, the
    only way to packed fused rows wider than 16 words."""

    def _launch_binned(self, keys_gpu, bins_gpu, out_gpu, scratch=None):
        b = len(keys_gpu)
        ew = self._fused_entry_words()
        stream, sptr, sbytes = self._launch_args(
            keys_gpu, (b, self.KEY_INTS), out_gpu, (b, ew), scratch)
        _check_arg("bins", bins_gpu, self._table_gpu.device, torch.int32, (b,))
        _hip.eval_fused_packed_binned(
            keys_gpu.data_ptr(), self._table_gpu.data_ptr(),
            bins_gpu.data_ptr(), out_gpu.data_ptr(), self._aes_ptr, b,
            self._n_domain, self._depth, self._zlog, self.num_bins,
            self.prf_method, stream, sptr, sbytes, ew)

    def __repr__(self):
        return "Packed" + super().__repr__()
