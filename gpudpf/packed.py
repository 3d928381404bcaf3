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

Not built, and refused: packed keys with bins (BinnedDPF), fused rows wider
than 16 words (they take the two-stage path), sharding (ShardedDPF), the
"bfs" and "coop" strategies, and the HTTP server.
"""

import torch

from gpudpf import _core
from gpudpf.dpf import DPF, _hip


class PackedDPF(DPF):
    LANE_LOG = _core.PACKED_LANE_LOG        # 2: four lanes
    MIN_DOMAIN = _core.PACKED_MIN_DOMAIN    # 512: tree depth >= 7

    def __init__(self, prf=None, device=None, fused_words=16):
        if fused_words != self.ENTRY_SIZE:
            raise Exception(
                "the packed fused kernel serves rows of at most %d words "
                "(got fused_words=%r); wider tables take the two-stage path"
                % (self.ENTRY_SIZE, fused_words))
        super().__init__(prf=prf, device=device, fused_words=fused_words)

    @staticmethod
    def _domain(n):
        """Next power of two >= 512: the tree over the n / 4 nodes keeps
        the depth >= 7 the kernels need."""
        d = PackedDPF.MIN_DOMAIN
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
