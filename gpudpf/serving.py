"""Production serving helpers.

GraphedServer: a hipGraph-captured serving step for fixed-batch key
streams — the launch-bound inner loop is captured once with
torch.cuda.CUDAGraph (hipGraph on ROCm) and replayed per batch, leaving
only the key H2D copy and result D2H on the host path.  This is the
idiomatic MI355X replacement for the reference's per-call stream
creation (dpf_wrapper.cu:155-156).

Serves all backend shapes:
  * fused (entry <= 16 words, or <= the DPF's fused_words): one captured
    zero+fused launch;
  * wide entries: captured expand + streaming-GEMM sequence (the MFMA
    digit-plane path allocates per call and is not graph-capturable;
    the streaming GEMM reads the table in place, so the whole two-stage
    pipeline replays from one graph);
  * ShardedDPF: the local fused partial is graph-replayed and the RCCL
    all-reduce runs outside the graph (collectives are not captured).

Measured at batch=512 the fused graph is throughput-NEUTRAL vs plain
launches (0.58 vs 0.55 ms at n=16384): ROCm launch overhead for a single
fused kernel is already small.  The value is the pinned, preallocated,
fixed-address serving loop, and launch-count amortization for the
multi-launch wide path.
"""

import torch

from gpudpf import ops
from gpudpf.dpf import DPF, as_key_batch


def _table_device(dpf):
    if dpf._table_gpu is None:
        raise Exception("eval_init the DPF before building a server")
    return dpf._table_gpu.device


class _Slot:
    """Fixed-address buffers, stream and events of one in-flight batch.
    `scratch` is the slot's own sibling-stack scratch (None: the shared
    per-device buffer); `shares` exists on the wide (two-stage) paths."""

    __slots__ = ("stream", "keys_pinned", "keys_gpu", "scratch", "shares",
                 "out_gpu", "out_pinned", "graph", "expanded", "done", "busy")

    def __init__(self, dpf, batch, stream=None, own_scratch=False,
                 shares=False, out_pinned=False):
        dev = dpf._table_gpu.device

        def zeros(cols, **kw):
            return torch.zeros((batch, cols), dtype=torch.int32, **kw)

        self.stream = stream
        self.keys_pinned = zeros(DPF.KEY_INTS).pin_memory()
        self.keys_gpu = zeros(DPF.KEY_INTS, device=dev)
        self.scratch = torch.empty(dpf._scratch_bytes(batch), dtype=torch.uint8,
                                   device=dev) if own_scratch else None
        self.shares = zeros(dpf._n_domain, device=dev) if shares else None
        self.out_gpu = zeros(dpf._entry_padded, device=dev)
        self.out_pinned = zeros(dpf._entry_padded).pin_memory() \
            if out_pinned else None
        self.graph = None
        self.expanded = torch.cuda.Event()
        self.done = torch.cuda.Event()
        self.busy = False

    def stage(self, keys):
        """Checked [batch, 524] CPU keys -> keys_gpu, on the current
        stream."""
        # raw memcpy into the pinned staging buffer: torch's copy_ into a
        # pinned tensor device-synchronizes when an async H2D from it is
        # still pending (measured 5+ ms); numpy assignment does not.
        self.keys_pinned.numpy()[:] = keys.numpy()
        self.keys_gpu.copy_(self.keys_pinned, non_blocking=True)

    def wait(self):
        self.done.synchronize()
        self.busy = False


def _fixed_batch(srv, keys):
    keys = as_key_batch(keys)
    if keys.shape[0] != srv.batch:
        raise Exception("%s is fixed at batch=%d"
                        % (type(srv).__name__, srv.batch))
    return keys


def _take_slot(srv):
    """Next slot of a pipelined server, round-robin; blocks only if the
    slot's previous batch was never collected."""
    slot = srv._slots[srv._next]
    srv._next = (srv._next + 1) % srv.depth
    if slot.busy:
        slot.wait()
    return slot


def _capture(launch, dev, stream=None):
    """Warm `launch` up on a side stream, then capture it into a graph."""
    warm = torch.cuda.Stream(dev)
    warm.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(warm):
        for _ in range(3):
            launch()
    torch.cuda.current_stream(dev).wait_stream(warm)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    # thread_local: the default 'global' capture mode errors ANY other
    # thread's CUDA call during capture — under a nccl process group
    # the RCCL watchdog thread races that window
    with torch.cuda.graph(graph, stream=stream,
                          capture_error_mode="thread_local"):
        launch()
    return graph


class GraphedServer:
    """Fixed-batch PIR serving loop with hipGraph replay.

    Usage:
        srv = GraphedServer(dpf, batch=512)   # dpf already eval_init'ed
        shares = srv.eval(keys_cpu)           # [batch, e] int32 (CPU)

    `dpf` may be a DPF or a ShardedDPF (then keys passed to eval must be
    full-domain keys; the subkey restriction runs on the host and the
    partial-sum all-reduce runs after graph replay).
    """

    MAX_WIDE_SHARES_BYTES = 16 << 30

    def __init__(self, dpf, batch: int):
        self.sharded = None
        if hasattr(dpf, "local"):  # ShardedDPF
            self.sharded = dpf
            dpf = dpf.local
        self.device = _table_device(dpf)
        self.dpf = dpf
        self.batch = batch
        self.wide = not dpf.fused_servable
        if self.sharded is not None and self.wide:
            raise Exception("sharded GraphedServer serves the fused path "
                            "(entry <= %d words)" % dpf.fused_words)
        if self.wide:
            shares_bytes = batch * dpf._n_domain * 4
            if shares_bytes > self.MAX_WIDE_SHARES_BYTES:
                raise Exception(
                    "wide GraphedServer share buffer would need %d bytes "
                    "(> %d); lower the batch" %
                    (shares_bytes, self.MAX_WIDE_SHARES_BYTES))
        # one step is in flight at a time: the shared scratch serves
        slot = self._slot = _Slot(dpf, batch, shares=self.wide)

        def launch():
            if self.wide:
                dpf._launch_expand(slot.keys_gpu, slot.shares)
                ops.pir_matmul_u32_stream(slot.shares, dpf._table_gpu,
                                          out=slot.out_gpu)
            else:
                slot.out_gpu.zero_()
                dpf._launch_fused(slot.keys_gpu, slot.out_gpu)

        self._graph = _capture(launch, self.device)

    def eval(self, keys, to_host=True):
        """keys: [batch, 524] int32 CPU tensor (or list) — full-domain
        keys for a sharded server, which restricts them per rank.
        Returns [batch, e] shares (CPU by default)."""
        keys = _fixed_batch(self, keys)
        if self.sharded is not None:
            keys = self.sharded.shard_subkeys(keys)
        self._slot.stage(keys)
        self._graph.replay()
        out = self._slot.out_gpu
        if self.sharded is not None:
            out = self.sharded._allreduce_(out)
        out = out[:, : self.dpf.table_effective_entry_size]
        return out.cpu() if to_host else out


class PipelinedServer:
    """Double-buffered throughput serving: batch i+1's host staging and
    H2D copy overlap batch i's kernel (the reference's own benchmark
    interleaves iterations on two CUDA streams the same way,
    dpf_benchmark.cu:191-231).  At small n the fused kernel is ~0.15 ms
    while key staging costs ~0.25 ms of host/copy time — the pipeline
    hides it.

    Usage (throughput loop):
        srv = PipelinedServer(dpf, batch=512)     # dpf eval_init'ed
        h = srv.submit(keys_cpu)                  # non-blocking
        shares = srv.collect(h)                   # [batch, e] int32 CPU
    Submitting more than `depth` batches blocks until a slot drains.
    Each batch still performs the full step (key H2D, fused kernel,
    share D2H) — only ADJACENT batches overlap.
    """

    def __init__(self, dpf: DPF, batch: int, depth: int = 2):
        self.device = _table_device(dpf)
        if not dpf.fused_servable:
            raise Exception("PipelinedServer serves the fused path "
                            "(entry <= %d words)" % dpf.fused_words)
        self.dpf = dpf
        self.batch = batch
        self.depth = depth
        self._slots = []
        for _ in range(depth):
            # Adjacent batches' kernels are in flight together on the
            # slots' streams, so each slot owns its sibling-stack scratch:
            # on the shared per-device buffer equal-numbered workgroups of
            # the two kernels overwrite each other's stacks (n >= 2^16)
            # and the shares come out wrong.
            slot = _Slot(dpf, batch, stream=torch.cuda.Stream(self.device),
                         own_scratch=True, out_pinned=True)

            def launch(s=slot):
                s.out_gpu.zero_()
                dpf._launch_fused(s.keys_gpu, s.out_gpu, s.scratch)

            slot.graph = _capture(launch, self.device, stream=slot.stream)
            self._slots.append(slot)
        self._next = 0

    def submit(self, keys):
        """Stage + launch a batch on the next slot (blocks only if the
        slot's previous batch has not been collected)."""
        keys = _fixed_batch(self, keys)
        slot = _take_slot(self)
        with torch.cuda.stream(slot.stream):
            slot.stage(keys)
            slot.graph.replay()
            slot.out_pinned.copy_(slot.out_gpu, non_blocking=True)
            slot.done.record(slot.stream)
        slot.busy = True
        return slot

    def collect(self, slot):
        """Wait for a submitted batch and return its [batch, e] shares."""
        slot.wait()
        return slot.out_pinned[:, : self.dpf.table_effective_entry_size
                               ].clone()


class TwoStageServer:
    """Pipelined wide-entry serving (entry > 16 words): batch i+1's
    one-hot expansion runs on its own stream while batch i's streaming
    GEMM reads the table — steady-state step = max(expansion, GEMM)
    instead of their sum.  On a 240 GB table (2^28 x 224) the serial
    two-stage step is ~53 ms expansion + ~64 ms GEMM; pipelined serving
    approaches the larger of the two.

    Usage:
        srv = TwoStageServer(dpf, batch=8)   # dpf eval_init'ed, wide
        h = srv.submit(keys_cpu)             # non-blocking
        shares = srv.collect(h)              # [batch, e] int32 CPU
    """

    def __init__(self, dpf: DPF, batch: int, depth: int = 2):
        dev = self.device = _table_device(dpf)
        if dpf.fused_servable:
            raise Exception("TwoStageServer serves wide entries "
                            "(> %d words); use PipelinedServer"
                            % dpf.fused_words)
        if batch > 16:
            raise Exception("streaming-GEMM batch is capped at 16 per "
                            "table pass; lower the batch")
        self.dpf = dpf
        self.batch = batch
        self.depth = depth
        free, _total = torch.cuda.mem_get_info(dev)
        need = depth * batch * dpf._n_domain * 4
        if need > free - (2 << 30):
            raise Exception("pipeline share buffers need %d bytes "
                            "(free %d); lower batch/depth" % (need, free))
        self._gemm_stream = torch.cuda.Stream(dev)
        # expansions of adjacent batches can overlap on the slots' streams:
        # per-slot sibling-stack scratch (see PipelinedServer)
        self._slots = [_Slot(dpf, batch, stream=torch.cuda.Stream(dev),
                             own_scratch=True, shares=True)
                       for _ in range(depth)]
        self._next = 0

    def submit(self, keys):
        keys = _fixed_batch(self, keys)
        slot = _take_slot(self)
        with torch.cuda.stream(slot.stream):
            slot.stage(keys)
            self.dpf._launch_expand(slot.keys_gpu, slot.shares, slot.scratch)
            slot.expanded.record(slot.stream)
        # the GEMM stream serializes table passes across slots (the table
        # stream is the contended resource); it only waits for THIS
        # slot's expansion
        self._gemm_stream.wait_event(slot.expanded)
        with torch.cuda.stream(self._gemm_stream):
            ops.pir_matmul_u32_stream(slot.shares, self.dpf._table_gpu,
                                      out=slot.out_gpu)
            slot.done.record(self._gemm_stream)
        slot.busy = True
        return slot

    def collect(self, slot):
        slot.wait()
        return slot.out_gpu[:, : self.dpf.table_effective_entry_size].cpu()
