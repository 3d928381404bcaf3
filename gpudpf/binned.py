"""Batch-PIR serving: one fused launch in which key i walks its own bin.

The batch-PIR plan (pir/batch_pir.py) hashes the cold part of a table into
`num_bins` small tables and sends `queries_per_bin` keys to every bin per
request, so a key costs bin_size PRFs, not n.  BinnedDPF holds all bins in
one device allocation, [num_bins, n, 16] (rows of up to 64 words with
fused_words, below) with every block in the kernel's leaf_perm order, and evaluates a batch whose key i belongs to bin bins[i]
with a single launch of the binned fused kernel (csrc/hip/dpf_eval.hip).

Every attribute the serving classes read keeps its meaning PER BIN
(_n_domain, _depth, _zlog, _entry_padded, table_effective_entry_size,
_scratch_bytes), and _launch_fused evaluates against the slot plan bound
with bind_bins, so GraphedServer and PipelinedServer serve a BinnedDPF
as they serve a DPF:

    d = BinnedDPF(prf=DPF.PRF_AES128)
    d.eval_init(tables)                  # list of [n_b, e] int32, e <= 16
    k1s, k2s = d.gen_batch(rows, bins)   # key i selects rows[i] of bins[i]
    d.bind_bins(bins)                    # the fixed slot plan, uploaded once
    shares = GraphedServer(d, batch=len(bins)).eval(k1s)

Bin rows wider than 16 words (a collocated plan's group_size * e) need
BinnedDPF(fused_words=32, 48 or 64): the fused kernel then walks rows of
that many words, still one launch and one leaf expansion per key.

gpudpf.PackedBinnedDPF (gpudpf/packed.py) is this class served with packed
keys, a quarter of the PRF blocks per key, at the same widths.
"""

import os

import numpy as np
import torch

from gpudpf import _core
from gpudpf.dpf import DPF, _check_arg, _hip, _HAS_HIP


class BinnedDPF(DPF):
    def __init__(self, prf=None, device=None, fused_words=16):
        super().__init__(prf=prf, device=device, fused_words=fused_words)
        self.tables = None      # natural-order bin tables (as given)
        self.bin_sizes = None   # rows of each bin
        self.num_bins = None
        self._perm = None       # natural -> row map of the common domain (CPU)
        self._plan = None       # bound slot plan: int32 [batch] bin ids

    # ------------------------------------------------------------------
    # Bins
    # ------------------------------------------------------------------
    def set_bin_sizes(self, sizes):
        """Declare the bins by their row counts (the client side, which has
        no tables; eval_init calls it).  The common key domain is
        DPF._domain(max size)."""
        sizes = [int(s) for s in sizes]
        if not sizes or min(sizes) < 1:
            raise Exception("need at least one bin and every bin >= 1 row "
                            "(got %s)" % sizes)
        self.bin_sizes = sizes
        self.num_bins = len(sizes)
        self._n_domain = self._domain(max(sizes))

    def _check_bins(self, bins):
        """An int sequence or CPU tensor of bin ids as a contiguous int32
        [m] CPU tensor; raises unless integer, 1-D and all in
        [0, num_bins)."""
        if self.num_bins is None:
            raise Exception("bins: call eval_init or set_bin_sizes first")
        t = bins if isinstance(bins, torch.Tensor) \
            else torch.as_tensor(np.asarray(bins))
        if t.device.type != "cpu":
            raise Exception("bins must be given on the host (got a tensor on "
                            "%s); bind_bins uploads them" % t.device)
        if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64,
                           torch.uint8):
            raise Exception("bins must be integers (got %s)" % t.dtype)
        if t.dim() != 1:
            raise Exception("bins must be 1-D (got shape %s)" % list(t.shape))
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.num_bins):
            raise Exception("bins must lie in [0, %d) (got min %d, max %d)"
                            % (self.num_bins, int(t.min()), int(t.max())))
        return t.to(torch.int32).contiguous()

    def bind_bins(self, bins):
        """Validate `bins` on the host and upload it as the slot plan that
        _launch_fused / eval_gpu_into / the servers evaluate against: key i
        of every later batch is evaluated against bin bins[i].  The only way
        bin ids reach the device, which cannot check them.  Returns the
        device tensor."""
        plan = self._check_bins(bins)
        if self._table_gpu is not None:
            plan = plan.to(self._table_gpu.device)
        self._plan = plan
        return plan

    # ------------------------------------------------------------------
    # Client side
    # ------------------------------------------------------------------
    def _check_row(self, k, b):
        if self.num_bins is None:
            raise Exception("call eval_init or set_bin_sizes before gen")
        if not 0 <= b < self.num_bins:
            raise Exception("bin %d out of range for %d bins"
                            % (b, self.num_bins))
        if not 0 <= k < self.bin_sizes[b]:
            raise Exception("k (%d) must be less than the %d rows of bin %d"
                            % (k, self.bin_sizes[b], b))

    def gen(self, k, bin):
        """The two server keys selecting row k of bin `bin` (keys of the
        common bin domain)."""
        self._check_row(int(k), int(bin))
        return super().gen(int(k), self._n_domain)

    def gen_batch(self, indices, bins):
        """Keys for rows indices[i] of bins[i].  Returns (k1s, k2s)
        int32[B,524] tensors."""
        indices = [int(k) for k in indices]
        bins = self._check_bins(bins).tolist()
        if len(indices) != len(bins):
            raise Exception("%d indices for %d bins"
                            % (len(indices), len(bins)))
        for k, b in zip(indices, bins):
            self._check_row(k, b)
        return super().gen_batch(indices, self._n_domain)

    # ------------------------------------------------------------------
    # Server side
    # ------------------------------------------------------------------
    def bin_block(self, b):
        """Bin b as the kernel reads it: [n, padded entry words] int32
        (CPU), zero-padded to the common domain and a multiple of 16 words,
        rows in leaf_perm(n, zlog) order."""
        t = self.tables[b]
        blk = torch.zeros((self._n_domain, self._entry_padded),
                          dtype=torch.int32)
        blk[self._perm[: t.shape[0]], : t.shape[1]] = t.to(torch.int32)
        return blk

    def eval_init(self, tables):
        """Upload a list of [n_b, e] int32 bin tables (every n_b >= 1, one
        e <= fused_words for all).  Bins are zero-padded to the common
        domain DPF._domain(max n_b) and each is reordered by leaf_perm; the
        device table is [num_bins, n, e padded to 16 words].  The upload
        streams in row chunks."""
        tables = list(tables)
        if not tables:
            raise Exception("need at least one bin table")
        for t in tables:
            if t.dim() != 2 or t.shape[0] < 1:
                raise Exception("every bin table must be [n_b >= 1, e] "
                                "(got %s)" % list(t.shape))
        es = sorted({int(t.shape[1]) for t in tables})
        if len(es) != 1:
            raise Exception("all bins must share one entry size (got %s)" % es)
        e = es[0]
        if e > self.fused_words:
            raise Exception("binned evaluation serves entries of at most %d "
                            "words (got %d): there is no binned two-stage path"
                            % (self.fused_words, e))
        self.tables = tables
        self.set_bin_sizes([t.shape[0] for t in tables])
        dev = self._setup_domain(max(self.bin_sizes), e)
        self._perm = self._perm_table()
        self._plan = None
        if dev.type != "cuda":
            self.eval_free()
            return
        self._table_gpu = torch.zeros(
            (self.num_bins, self._n_domain, self._entry_padded),
            dtype=torch.int32, device=dev)
        self._perm_gpu = self._perm.to(dev)
        if self.prf_method == self.PRF_AES128:
            self._aes_ptr = _hip.ensure_aes_tables(dev.index)
        rows_per_chunk = max(1, self.INIT_CHUNK_BYTES // (self._entry_padded * 4))
        for b, t in enumerate(tables):
            t32 = t.to(torch.int32)
            for lo in range(0, t.shape[0], rows_per_chunk):
                hi = min(t.shape[0], lo + rows_per_chunk)
                self._table_gpu[b, self._perm_gpu[lo:hi], :e] = \
                    t32[lo:hi].to(dev, non_blocking=False)

    def _launch_binned(self, keys_gpu, bins_gpu, out_gpu, scratch=None):
        """out_gpu [b, padded entry words] += share of key i against bin
        bins_gpu[i]; the caller zeroes it.  Metadata checks only:
        capture-safe."""
        b = len(keys_gpu)
        ew = self._fused_entry_words()
        stream, sptr, sbytes = self._launch_args(
            keys_gpu, (b, self.KEY_INTS), out_gpu, (b, ew), scratch)
        _check_arg("bins", bins_gpu, self._table_gpu.device, torch.int32, (b,))
        _hip.eval_fused_binned(
            keys_gpu.data_ptr(), self._table_gpu.data_ptr(),
            bins_gpu.data_ptr(), out_gpu.data_ptr(), self._aes_ptr, b,
            self._n_domain, self._depth, self._zlog, self.num_bins,
            self.prf_method, stream, sptr, sbytes, ew)

    def _launch_fused(self, keys_gpu, out_gpu, scratch=None):
        """As DPF._launch_fused, key i against bin plan[i] of the plan bound
        with bind_bins."""
        if self._plan is None:
            raise Exception("bins: call bind_bins before launching (no slot "
                            "plan is bound)")
        if len(self._plan) != len(keys_gpu):
            raise Exception("bins: the bound plan has %d slots but the batch "
                            "has %d keys" % (len(self._plan), len(keys_gpu)))
        self._launch_binned(keys_gpu, self._plan, out_gpu, scratch)

    def eval_gpu(self, keys, bins, one_hot_only=False, strategy="fused",
                 out_device=False):
        """Evaluate key i against bin bins[i] on the GPU.  Returns
        [batch, e] int32 shares.  The bound slot plan is left alone."""
        if one_hot_only:
            raise NotImplementedError("binned one-hot output is not built")
        if strategy != "fused":
            raise NotImplementedError(
                "binned evaluation has the fused strategy only (got %r)"
                % (strategy,))
        if self._table_gpu is None:
            raise Exception("Must call `eval_init` before `eval_gpu`")
        if not _HAS_HIP:
            raise Exception("gpudpf._hip extension is not available")
        kt, n, _depth = self._keys_tensor(keys)
        if n != self._n_domain:
            raise Exception("key domain (%d) does not match bin domain (%d)"
                            % (n, self._n_domain))
        bt = self._check_bins(bins)
        if len(bt) != len(kt):
            raise Exception("bins: %d ids for %d keys" % (len(bt), len(kt)))
        dev = self._table_gpu.device
        keys_gpu = kt.to(dev, non_blocking=True)
        bins_gpu = bt.to(dev, non_blocking=True)
        outs = []
        for lo in range(0, len(keys_gpu), self.MAX_LAUNCH_BATCH):
            ks = keys_gpu[lo:lo + self.MAX_LAUNCH_BATCH]
            out = self._new_out(len(ks), one_hot=False)
            self._launch_binned(ks, bins_gpu[lo:lo + self.MAX_LAUNCH_BATCH],
                                out)
            outs.append(out)
        res = torch.cat(outs) if len(outs) > 1 else outs[0]
        res = res[:, : self.table_effective_entry_size]
        return res if out_device else res.cpu()

    def eval_cpu(self, keys, bins, num_threads=None):
        """CPU reference: key i against the natural-order table of bin
        bins[i]."""
        if self.tables is None:
            raise Exception("Must call `eval_init` before `eval_cpu`")
        kt, n, _depth = self._keys_tensor(keys)
        if n != self._n_domain:
            raise Exception("key domain (%d) does not match bin domain (%d)"
                            % (n, self._n_domain))
        bt = self._check_bins(bins).tolist()
        if len(bt) != len(kt):
            raise Exception("bins: %d ids for %d keys" % (len(bt), len(kt)))
        if num_threads is None:
            num_threads = min(32, os.cpu_count() or 1)
        arrs = [kt[i].numpy() for i in range(kt.shape[0])]
        one_hots = torch.from_numpy(
            np.asarray(_core.expand_batch(arrs, self.prf_method, num_threads)))
        out = torch.zeros((len(bt), self.table_effective_entry_size),
                          dtype=torch.int32)
        for i, b in enumerate(bt):
            t = self.tables[b]
            out[i] = torch.matmul(one_hots[i, : t.shape[0]].to(torch.int64),
                                  t.to(torch.int64)).to(torch.int32)
        return out

    # ------------------------------------------------------------------
    # What a binned table does not serve
    # ------------------------------------------------------------------
    def eval_init_empty(self, n, e):
        raise NotImplementedError("binned tables are uploaded by eval_init")

    def table_write(self, indices, rows):
        raise NotImplementedError("binned tables have no streaming ingest")

    def table_read(self, indices):
        raise NotImplementedError("binned tables have no row gather")

    def eval_free(self):
        super().eval_free()
        self._plan = None

    def __repr__(self):
        if self.tables is None:
            return "BinnedDPF(_uninitialized_, prf_method=%s)" \
                % self.prf_method_string
        return "BinnedDPF(bins=%d, bin_domain=%d, entry_size=%d, " \
            "prf_method=%s)" % (self.num_bins, self._n_domain,
                                self.table_effective_entry_size,
                                self.prf_method_string)
