"""Direct intra-node all-reduce over xGMI for the flat gradient buffer.

RCCL's ring moves every byte around the 8 GPUs over one link per direction per ring. On an MI355X
node every GPU has a direct xGMI link to each of its 7 peers, so this backend works per link
instead. Default engine (``csrc/comm/xgmi.cpp`` XgmiEngine, native):

* reduce-scatter: rank r owns slice r of each bucket; ONE pull-reduce kernel reads slice r from
  every rank's IPC-mapped gradient buffer (the 7 peers' over their xGMI links at once) and sums them
  in fp32 in rank order into its own buffer: one rounding, so every rank gets bit-identical values,
  deterministically, and no staging copy;
* all-gather: ONE pull-gather kernel copies every owner's reduced slice into this rank's buffer;
* both kernels run on one high-priority comm stream, scheduled by a C++ worker thread, so the
  backward thread only records an event and enqueues the bucket (no Python in the critical window,
  one hardware queue for all of it).

Per bucket, the traffic per link is bucket/W per phase. (Round 4's copy-engine path -- one copy
stream per peer into local staging, then the reduction kernel, orchestrated by a Python thread -- was
replaced by this engine and removed in round 6.)

Cross-process ordering uses interprocess HIP events only: a rank's comm stream waits, on the GPU,
on its peers' "bucket ready" / "slice reduced" events, and no kernel spins. The host only
guarantees that an event was recorded (for THIS step) before anyone waits on it: every rank
publishes a per-bucket sequence number in a page of host shared memory right after recording, and
the worker of a peer polls that word (microseconds). The backward thread never blocks.

Sharded optimizer (``GradReducer(shard=True)``): the reduce-scatter is the pull-reduce alone, and
after the AdamW update of the owned slice one pull-gather per bucket copies the peers' updated
slices from their IPC-mapped PARAMETER buffers (:meth:`XgmiAllReduce.gather`; a third per-bucket
event and sequence word, "updated"). Sparse embedding exchange: the ranks publish their sorted token
ids in a small IPC-mapped list, and two kernels reduce the union's rows in place in the mapped dense
gradients, each row by the rank that owns its row range (:meth:`XgmiAllReduce.launch_sparse`,
``csrc/kernels/comm.hip`` sparse_rows_kernel). The ordering argument is in ``csrc/comm/xgmi.cpp``.

The gradient buffer is reallocated with ``hipMalloc`` so it can be exported with
``hipIpcGetMemHandle``. Opt-in: ``GradReducer(..., backend="xgmi")``, ``train.py --allreduce
xgmi``, ``bench.py --allreduce xgmi``. RCCL stays the default.
"""
from __future__ import annotations

import os
import time
import uuid
from multiprocessing import shared_memory
from typing import List, Sequence, Tuple

import numpy as np

import torch
import torch.distributed as dist

from .. import _ext



def _device_identity(i: int) -> str:
    """Stable identity of visible device i across processes (UUID, else PCI address)."""
    p = torch.cuda.get_device_properties(i)
    u = getattr(p, "uuid", None)
    if u is not None and str(u).strip("0-") != "":
        return str(u)
    pci = tuple(getattr(p, a, None) for a in ("pci_domain_id", "pci_bus_id", "pci_device_id"))
    if any(x is not None for x in pci):
        return "pci:%s:%s:%s" % pci
    return f"{p.name}#{i}"


def _hidden_ranks(vis) -> List[int]:
    """Ranks whose GPU some rank cannot see; vis[r] = (rank r's device identity, identities rank r sees)."""
    return sorted({r for r, (own, _) in enumerate(vis) for _, seen in vis if own not in seen})

def slice_cuts(lo: int, hi: int, world: int) -> List[int]:
    """The engine's W + 1 cuts of bucket [lo, hi): rank r reduces [cuts[r], cuts[r + 1]) (8-element =
    16-B aligned boundaries, the remainder in the last slice)."""
    n = hi - lo
    return [lo + ((n * r // world) // 8) * 8 for r in range(world)] + [hi]


def sharded_slices(ranges: Sequence[Tuple[int, int]], world: int) -> List[List[Tuple[int, int]]]:
    """The engine's slices of every bucket for the sharded optimizer, checked: bucket b must be W
    equal 64-element-aligned chunks (``FlatParams.relayout``'s padded layout), and then slice r is
    exactly chunk r, ``GradReducer.owned(b)`` of rank r. Anything else is rejected: the optimizer
    would update elements whose reduced gradient this rank does not hold."""
    out = []
    for b, (lo, hi) in enumerate(ranges):
        n = hi - lo
        if n <= 0 or n % (64 * world) or lo % 64:
            raise ValueError(f"xgmi sharded optimizer: bucket {b} [{lo}, {hi}) is not {world} equal 64-element-aligned "
                             "chunks (an unpadded layout: build the GradReducer before the optimizer)")
        c = n // world
        cuts = slice_cuts(lo, hi, world)
        sl = [(cuts[r], cuts[r + 1]) for r in range(world)]
        if sl != [(lo + r * c, lo + (r + 1) * c) for r in range(world)]:
            raise ValueError(f"xgmi sharded optimizer: bucket {b}: the engine's slices {sl} are not the owned chunks")
        out.append(sl)
    return out


class _Work:
    __slots__ = ("owner", "b", "seq")

    def __init__(self, owner, b):
        self.owner = owner
        self.b = b
        self.seq = 0  # the step this bucket belongs to (a ticket for wait)

    def wait(self):
        """Current stream waits (GPU-side) for the all-reduced bucket."""
        self.owner.eng.wait(self.b, self.seq, torch.cuda.current_stream(self.owner.dev).cuda_stream)


class _GatherWork(_Work):
    __slots__ = ()

    def wait(self):
        """Current stream waits (GPU-side) for the bucket's parameter all-gather."""
        self.owner.eng.wait_gather(self.b, self.seq, torch.cuda.current_stream(self.owner.dev).cuda_stream)


class _HostSeq:
    """[world, slots] int64 sequence words in one POSIX shared-memory page set (node-local ranks):
    rank r publishes ``seq`` in its own row; readers poll a peer's word until it reaches ``seq``.
    Aligned 8-byte stores/loads are single-copy atomic on x86-64."""

    def __init__(self, rank: int, world: int, slots: int, group):
        name = [f"pra_xgmi_{uuid.uuid4().hex[:16]}" if rank == 0 else None]
        dist.broadcast_object_list(name, src=0, group=group)
        size = world * slots * 8
        self.owner = rank == 0
        if self.owner:
            self.shm = shared_memory.SharedMemory(name=name[0], create=True, size=size)
        dist.barrier(group=group)
        if not self.owner:
            self.shm = shared_memory.SharedMemory(name=name[0], create=False, size=size)
            # Python < 3.13 registers attached segments with the resource tracker too, which would
            # unlink rank 0's segment when this process exits; only the creator owns it
            from multiprocessing import resource_tracker

            resource_tracker.unregister(self.shm._name, "shared_memory")
        else:
            import atexit

            atexit.register(self.close)  # never leave the page behind in /dev/shm
        self.a = np.ndarray((world, slots), dtype=np.int64, buffer=self.shm.buf)
        if self.owner:
            self.a[:] = 0
        dist.barrier(group=group)
        self.rank = rank

    def publish(self, slot: int, seq: int):
        self.a[self.rank, slot] = seq

    def wait(self, r: int, slot: int, seq: int, timeout: float = 600.0):
        """Poll rank r's word until it reaches seq (the host side of the engine's wait_word)."""
        if self.a[r, slot] >= seq:
            return
        t0 = time.perf_counter()
        spins = 0
        while self.a[r, slot] < seq:
            spins += 1
            if spins > 200:
                time.sleep(20e-6)
            if time.perf_counter() - t0 > timeout:
                raise TimeoutError(f"xgmi: rank {r} did not publish slot {slot} seq {seq}")

    def address(self) -> int:
        """Base address of the [world, slots] int64 words in this process (for the native engine)."""
        return self.a.ctypes.data

    def close(self):
        if getattr(self, "a", None) is None:
            return
        self.a = None
        self.shm.close()
        if self.owner:
            try:
                self.shm.unlink()
            except FileNotFoundError:
                pass


class XgmiAllReduce:
    """``shard=True`` (the sharded optimizer): a bucket's launch is the reduce-scatter alone (this
    rank's slice, :func:`sharded_slices`), and :meth:`gather` pulls the peers' updated parameter slices;
    for that the flat PARAMETER buffer is reallocated IPC-exportable too and mapped into the peers."""

    def __init__(self, flat, ranges: Sequence[Tuple[int, int]], group=None, shard: bool = False):
        self.C = _ext.native().xgmi
        self.shard = bool(shard)
        self.ranges = list(ranges)
        # sharded: rejected here, before any allocation or collective (every rank raises alike)
        self.slices = (sharded_slices(self.ranges, dist.get_world_size(group)) if self.shard else None)
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = W = dist.get_world_size(group)
        if not 1 < W <= 16:
            raise ValueError("xgmi all-reduce needs 2..16 ranks on one node")
        self.flat = flat
        self.dev = flat.grad.device
        di = self.dev.index
        self.dtype = flat.grad.dtype
        self.esz = flat.grad.element_size()
        # 1) CPU barriers for the comm thread (its own gloo group, used by nothing else)
        self.hgroup = dist.new_group(backend="gloo")
        # 2) every peer GPU must be visible to map its buffer: under SLURM per-task isolation
        # (--gpus-per-task=1 / --gpu-bind) each rank sees only its own device and peer IPC cannot
        # work. Devices are compared by identity (UUID / PCI address), not by index, so ranks that
        # share one GPU (one-GPU rehearsals) pass and isolated ranks that all see "device 0" do not.
        # Decided collectively, so every rank raises instead of one rank hanging the others.
        n_vis = torch.cuda.device_count()
        mine = (_device_identity(di), [_device_identity(i) for i in range(n_vis)])
        vis: List = [None] * W
        dist.all_gather_object(vis, mine, group=self.hgroup)
        hidden = _hidden_ranks(vis)
        if hidden:
            raise RuntimeError(
                f"xgmi all-reduce needs every rank's GPU visible to every rank (GPUs of ranks {hidden} are "
                f"hidden from some peers; visible per rank: {[len(s) for _, s in vis]}); per-task GPU "
                "isolation (srun --gpus-per-task=1 / --gpu-bind, or per-rank ROCR_VISIBLE_DEVICES) hides "
                "the peers. Use the default RCCL all-reduce (--allreduce rccl) or launch with every GPU "
                "visible.")
        # 3) exportable gradient buffer
        buf = self.C.ipc_empty(flat.grad.numel(), self.dtype, di)
        buf.copy_(flat.grad)
        flat.rebind_grad(buf)
        self.buf = buf
        # sharded: the parameter buffer too (FlatParams.relayout just reallocated it, no optimizer is
        # bound yet), so a peer pulls this rank's updated slice straight from it
        self.pbuf = None
        if self.shard:
            if flat.data.dtype != self.dtype or flat.data.numel() != flat.grad.numel():
                raise ValueError("xgmi sharded optimizer: parameters and gradients must share dtype and layout")
            self.pbuf = self.C.ipc_empty(flat.data.numel(), flat.data.dtype, di)
            flat.rebind_data(self.pbuf)
        # 4) peer buffers (a failed open is reported on every rank)
        self.peer_base = self._map_peers(buf, "gradient")
        self.peer_pbase = self._map_peers(self.pbuf, "parameter") if self.shard else []
        # 4) slices (identical on every rank; 8-element = 16-B aligned boundaries)
        if self.slices is None:
            self.slices = []
            for lo, hi in self.ranges:
                cuts = slice_cuts(lo, hi, W)
                self.slices.append([(cuts[r], cuts[r + 1]) for r in range(W)])
        # 5) events: per bucket "ready" and "reduced" (and, sharded, "updated"; interprocess), one
        # per-step "done"
        nb = len(self.ranges)
        self.ev_ready = [self.C.ipc_event_create(di) for _ in range(nb)]
        self.ev_rs = [self.C.ipc_event_create(di) for _ in range(nb)]
        self.ev_upd = [self.C.ipc_event_create(di) for _ in range(nb)] if self.shard else []
        self.ev_step = self.C.ipc_event_create(di)
        mine = ([self.C.ipc_event_handle(e) for e in self.ev_ready], [self.C.ipc_event_handle(e) for e in self.ev_rs],
                self.C.ipc_event_handle(self.ev_step), [self.C.ipc_event_handle(e) for e in self.ev_upd])
        allh: List = [None] * W
        dist.all_gather_object(allh, mine, group=self.hgroup)
        self.peer_ready, self.peer_rs, self.peer_step, self.peer_upd = [], [], [], []
        for r in range(W):
            if r == self.rank:
                self.peer_ready.append(self.ev_ready)
                self.peer_rs.append(self.ev_rs)
                self.peer_step.append(self.ev_step)
                self.peer_upd.append(self.ev_upd)
            else:
                self.peer_ready.append([self.C.ipc_event_open(h, di) for h in allh[r][0]])
                self.peer_rs.append([self.C.ipc_event_open(h, di) for h in allh[r][1]])
                self.peer_step.append(self.C.ipc_event_open(allh[r][2], di))
                self.peer_upd.append([self.C.ipc_event_open(h, di) for h in allh[r][3]])
        # 6) host sequence words: [ready b | reduced b | updated b | step]
        self.nb = nb
        self.seq = 1  # current step's sequence number (published values start at 1)
        self.hseq = _HostSeq(self.rank, W, self.C.XgmiEngine.words_per_rank(nb), self.hgroup)
        # the native engine (csrc/comm/xgmi.cpp XgmiEngine): one comm stream, one pull-reduce kernel
        # reading every peer's slice over xGMI and one pull-gather kernel per bucket, scheduled by a
        # C++ worker thread
        code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[self.dtype]
        cuts = [c for sl in self.slices for c in [s0 for s0, _ in sl] + [sl[-1][1]]]
        self.eng = self.C.XgmiEngine(
            di, self.rank, W, code, self.esz, list(self.peer_base), cuts, self.hseq.address(),
            list(self.ev_ready), list(self.ev_rs), self.ev_step,
            [e for r in range(W) for e in self.peer_ready[r]], [e for r in range(W) for e in self.peer_rs[r]],
            list(self.peer_step), list(self.peer_pbase), list(self.ev_upd),
            [e for r in range(W) for e in self.peer_upd[r]] if self.shard else [])
        self.ids_buf = None  # sparse exchange: this rank's published id list (allocated at first use)
        dist.barrier(group=self.hgroup)

    def _map_peers(self, buf: torch.Tensor, what: str) -> List[int]:
        """Exchange ``buf``'s IPC handle and map every peer's buffer; a failed open is reported on
        every rank. Returns the W base addresses (this rank's own at index rank)."""
        W, di = self.world, self.dev.index
        handles: List = [None] * W
        dist.all_gather_object(handles, self.C.ipc_mem_handle(buf), group=self.hgroup)
        out, err = [], None
        for r in range(W):
            if r == self.rank:
                out.append(buf.data_ptr())
                continue
            try:
                out.append(self.C.ipc_open_mem(handles[r], di))
            except RuntimeError as e:  # noqa: PERF203
                err = f"rank {self.rank}: ipc_open_mem of rank {r}'s buffer failed: {e}"
                break
        errs: List = [None] * W
        dist.all_gather_object(errs, err, group=self.hgroup)
        bad = [e for e in errs if e]
        if bad:
            raise RuntimeError(f"xgmi all-reduce cannot map peer {what} buffers (GPU isolation or no "
                               "dmabuf IPC; HSA_ENABLE_IPC_MODE_LEGACY=0 is required): " + "; ".join(bad))
        return out

    # --- backward thread -----------------------------------------------------------------
    def launch(self, b: int) -> _Work:
        w = _Work(self, b)
        w.seq = self.eng.launch(b, torch.cuda.current_stream(self.dev).cuda_stream)
        return w

    def gather(self, b: int) -> _GatherWork:
        """Sharded: bucket b's owned parameter slice was updated on the current stream; pull the
        peers' updated slices behind it (one pull-gather on the comm stream)."""
        w = _GatherWork(self, b)
        w.seq = self.eng.gather(b, torch.cuda.current_stream(self.dev).cuda_stream)
        return w

    def launch_sparse(self, b: int, slot, vocab: int) -> _Work:
        """Bucket b holds only ``slot``, a [vocab, D] embedding gradient whose non-zero rows are those
        of ``slot.sparse_ids``: publish the ids, sorted (fixed size, duplicates kept, no host sync for
        a count), in an IPC-mapped list and reduce the union's rows in place (XgmiEngine, sparse
        bucket). The list is allocated, and mapped into the peers, at the first step: a collective,
        every rank gets here in the same backward. Later steps may bring fewer ids (the tail is filled
        with ``vocab``, which the kernel skips as out of range), never more."""
        ids = getattr(slot, "sparse_ids", None)
        if ids is None:
            raise RuntimeError("sparse embedding exchange: the embedding backward recorded no token ids")
        s, _ = torch.sort(ids.reshape(-1).to(torch.int64))
        n = s.numel()
        if self.ids_buf is None:
            ns: List = [None] * self.world
            dist.all_gather_object(ns, n, group=self.hgroup)
            if len(set(ns)) != 1 or n == 0:
                raise RuntimeError(f"sparse embedding exchange: the ranks' token counts per step differ: {ns}")
            D = slot.numel // vocab
            if D * vocab != slot.numel or D % 8:
                raise ValueError(f"sparse embedding exchange on xgmi: the embedding width {D} must be a multiple of 8")
            self.ids_buf = self.C.ipc_empty(n, torch.int64, self.dev.index)
            self.peer_ids = self._map_peers(self.ids_buf, "token id")
            self.eng.set_sparse(b, slot.offset, vocab, D, n, list(self.peer_ids))
        cap = self.ids_buf.numel()
        if n > cap:
            raise RuntimeError(f"sparse embedding exchange: {n} token ids this step, the list was sized for {cap}")
        self.ids_buf[:n].copy_(s)
        if n < cap:
            self.ids_buf[n:].fill_(vocab)
        slot.sparse_ids = None
        return self.launch(b)

    def end_step(self):
        """After every bucket of the step was waited on: no rank may overwrite its gradient
        buffer (next backward) before every peer finished reading it."""
        self.eng.end_step(torch.cuda.current_stream(self.dev).cuda_stream)
        self.seq += 1
