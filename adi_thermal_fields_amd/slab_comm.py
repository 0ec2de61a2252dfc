"""slab_comm -- how the ranks of a slab decomposition talk (dist_slab.SlabStepper's `comm`): the product transport over
torch.distributed (nccl = RCCL over xGMI), the test and rehearsal transports, and the helpers around them (slab sizes, the
environment RCCL wants, gathering the slabs on rank 0).  A comm has `rank`, `world`, `exchange_planes` and `all_gather`."""
import threading

import torch

__all__ = ['TorchDistComm', 'HostStagedDistComm', 'LocalComm', 'LoopbackComm', 'SelfLoopDistComm', 'split_planes',
           'rccl_env_defaults', 'gather_slabs']


def rccl_env_defaults():
    """Environment a rank wants BEFORE `init_process_group('nccl')` (setdefault: the caller's own settings win).
    * HSA_ENABLE_IPC_MODE_LEGACY=0: the hosts of this pool only support dmabuf IPC.
    * TORCH_NCCL_HIGH_PRIORITY=1: torch runs RCCL kernels on an internal stream; at normal priority HIP may map that
      stream onto the same hardware queue as the stream the sweeps run on (measured: rocprofv3 showed both on one HSA
      queue), and then a halo send/recv posted "beside" a sweep runs after it instead -- nothing overlaps.  High-priority
      streams get queues of their own: per-rank step over the RCCL self-loop 1.65 -> 1.59 ms."""
    import os
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    os.environ.setdefault('TORCH_NCCL_HIGH_PRIORITY', '1')


def split_planes(nx, world):
    """Even slab sizes (the fast condensation kernel wants whole 2/4/8-row segments)."""
    base = (nx // world) // 2 * 2
    sizes = [base] * world
    rem = nx - base * world
    i = 0
    while rem >= 2:
        sizes[i % world] += 2
        rem -= 2
        i += 1
    sizes[-1] += rem
    assert sum(sizes) == nx and all(s > 0 for s in sizes), (nx, world, sizes)
    return sizes

class TorchDistComm:
    """torch.distributed (nccl = RCCL on ROCm, or gloo on CPU).

    all_gather_mode: how the all-gather of the interface forms that need every rank's planes ('exact', 'deferred_exact': thin
    slabs, strong scaling) travels.  'collective' = `all_gather_into_tensor` (RCCL picks its algorithm, ring-like on most
    topologies: world-1 steps, each bound by ONE link); 'mesh' = every rank sends its block to every other rank in one batch of
    point-to-point operations -- on an xGMI node every pair of GPUs has a link of its own (7 x ~153 GB/s per GPU), so the
    world-1 blocks leave over world-1 links at once; 'auto' (default) = measured: the first time a payload of a size class
    (>= 256 KiB, device tensors, nccl, world >= 3) comes by, both are timed on the spot (a few iterations each, the slower rank
    counts) and the faster one is kept for that size class.  The choice is collective -- it comes out of an all-reduce -- and is
    reported by bench.py in `ranks.all_gather`; nothing here has run on more than one GPU, which is why it is measured, not
    assumed."""

    def __init__(self, group=None, all_gather_mode='auto'):
        import torch.distributed as dist
        assert all_gather_mode in ('auto', 'collective', 'mesh')
        self.dist = dist
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.bytes_sent = 0          # payload this rank has handed to the transport (bench.py reports it per step)
        self.n_exchanges = 0
        self.all_gather_mode = all_gather_mode
        self.tune_min_bytes, self.tune_any_backend = 256 << 10, False        # (tests lower / set these to walk the measuring path on gloo)
        self.all_gather_choice = {}  # size class (bytes, rounded up to a power of two) -> dict(mode, collective_ms, mesh_ms)

    def exchange_planes(self, send_lo, send_hi, recv_lo, recv_hi):
        """send_lo -> rank-1 (received there as recv_hi), send_hi -> rank+1 (received there as recv_lo)."""
        dist = self.dist
        ops = []
        if self.rank > 0:
            ops.append(dist.P2POp(dist.isend, send_lo, self.rank - 1, self.group))
            ops.append(dist.P2POp(dist.irecv, recv_lo, self.rank - 1, self.group))
            self.bytes_sent += send_lo.numel() * send_lo.element_size()
        if self.rank < self.world - 1:
            ops.append(dist.P2POp(dist.isend, send_hi, self.rank + 1, self.group))
            ops.append(dist.P2POp(dist.irecv, recv_hi, self.rank + 1, self.group))
            self.bytes_sent += send_hi.numel() * send_hi.element_size()
        if ops:
            self.n_exchanges += 1
            for r in dist.batch_isend_irecv(ops):
                r.wait()

    def _all_gather_mesh(self, out, inp):
        """every block straight to every peer: world-1 sends and world-1 receives in ONE batch"""
        dist, n = self.dist, inp.numel()
        flat, src = out.view(-1), inp.reshape(-1)
        flat[self.rank * n:(self.rank + 1) * n].copy_(src)
        ops = []
        for d in range(1, self.world):                 # peers in rotated order: no two ranks start on the same target
            r = (self.rank + d) % self.world
            ops.append(dist.P2POp(dist.isend, src, r, self.group))
        for d in range(1, self.world):
            r = (self.rank - d) % self.world
            ops.append(dist.P2POp(dist.irecv, flat[r * n:(r + 1) * n], r, self.group))
        for w in dist.batch_isend_irecv(ops):
            w.wait()

    def _all_gather_pick(self, out, inp):
        """'collective' or 'mesh' for this payload (see the class docstring); measured once per size class when 'auto'"""
        if self.all_gather_mode != 'auto':
            return self.all_gather_mode
        nbytes = inp.numel() * inp.element_size()
        on_rccl = inp.is_cuda and self.dist.get_backend(self.group) == 'nccl'
        if nbytes < self.tune_min_bytes or self.world < 3 or not (on_rccl or self.tune_any_backend):
            return 'collective'
        cls = 1 << (nbytes - 1).bit_length()
        got = self.all_gather_choice.get(cls)
        if got is None:
            dist = self.dist
            times = []
            for fn in (lambda: dist.all_gather_into_tensor(out, inp, group=self.group), lambda: self._all_gather_mesh(out, inp)):
                for _ in range(2):
                    fn()
                if inp.is_cuda:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.current_stream().synchronize()
                    dist.barrier(group=self.group)
                    e0.record()
                    for _ in range(5):
                        fn()
                    e1.record(); e1.synchronize()
                    times.append(e0.elapsed_time(e1) / 5.0)
                else:
                    import time
                    dist.barrier(group=self.group)
                    t0 = time.perf_counter()
                    for _ in range(5):
                        fn()
                    times.append((time.perf_counter() - t0) * 1e3 / 5.0)
            t = torch.tensor(times, dtype=torch.float64, device=inp.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)          # the slowest rank counts; the same on every rank
            tc, tm = float(t[0]), float(t[1])
            got = self.all_gather_choice[cls] = dict(mode='mesh' if tm < 0.9 * tc else 'collective', collective_ms=round(tc, 4),
                                                     mesh_ms=round(tm, 4))
        return got['mode']

    def all_gather(self, out, inp):
        self.bytes_sent += inp.numel() * inp.element_size() * (self.world - 1)
        if self._all_gather_pick(out, inp) == 'mesh':
            self._all_gather_mesh(out, inp)
        else:
            self.dist.all_gather_into_tensor(out, inp, group=self.group)


class HostStagedDistComm(TorchDistComm):
    """A TEST transport, not a product path: torch.distributed 'gloo' between processes whose fields live on a GPU.  Every
    payload goes device -> pinned host buffer -> gloo -> pinned host buffer -> device, the copies on the CURRENT stream, so
    the stream / event ordering SlabStepper sets up around an exchange is the one a RCCL run has.  RCCL refuses a second rank
    on the same device, gloo does not care: with this transport several REAL processes -- separate HIP contexts, separate
    allocators, a real rendezvous -- drive HipEngine + SlabStepper on the one GPU of a test box
    (tests/test_dist_hip_processes.py, `bench.py --transport gloo-staged`)."""

    def __init__(self, group=None):
        super().__init__(group)
        self._pin = {}

    def _host(self, tag, t):
        key = (tag, tuple(t.shape), t.dtype)
        h = self._pin.get(key)
        if h is None:
            h = torch.zeros(tuple(t.shape), dtype=t.dtype).pin_memory() if t.is_cuda else torch.zeros(tuple(t.shape), dtype=t.dtype)
            self._pin[key] = h
        return h

    @staticmethod
    def _wait_stream(t):
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()

    def exchange_planes(self, send_lo, send_hi, recv_lo, recv_hi):
        dist, ops, back = self.dist, [], []
        if self.rank > 0:
            hs, hr = self._host('s_lo', send_lo), self._host('r_lo', recv_lo)
            hs.copy_(send_lo, non_blocking=True)
            ops += [dist.P2POp(dist.isend, hs, self.rank - 1, self.group), dist.P2POp(dist.irecv, hr, self.rank - 1, self.group)]
            back.append((recv_lo, hr))
            self.bytes_sent += send_lo.numel() * send_lo.element_size()
        if self.rank < self.world - 1:
            hs, hr = self._host('s_hi', send_hi), self._host('r_hi', recv_hi)
            hs.copy_(send_hi, non_blocking=True)
            ops += [dist.P2POp(dist.isend, hs, self.rank + 1, self.group), dist.P2POp(dist.irecv, hr, self.rank + 1, self.group)]
            back.append((recv_hi, hr))
            self.bytes_sent += send_hi.numel() * send_hi.element_size()
        if not ops:
            return
        self.n_exchanges += 1
        self._wait_stream(send_lo)
        for r in dist.batch_isend_irecv(ops):
            r.wait()
        for dst, h in back:
            dst.copy_(h, non_blocking=True)
        self._wait_stream(send_lo)       # the pinned buffers are reused by the next exchange, possibly issued on another stream

    def all_gather(self, out, inp):
        self.bytes_sent += inp.numel() * inp.element_size() * (self.world - 1)
        hi = self._host('ag_i', inp.reshape(-1))
        ho = self._host('ag_o', out.reshape(-1))
        hi.copy_(inp.reshape(-1), non_blocking=True)
        self._wait_stream(inp)
        self.dist.all_gather_into_tensor(ho, hi, group=self.group)
        out.view(-1).copy_(ho, non_blocking=True)
        self._wait_stream(inp)


def gather_slabs(local, sizes, group=None, host_staged=False):
    """The whole field on rank 0 (a tensor on `local`'s device; None on the other ranks) from slabs of sizes[r] planes each.
    Point-to-point copies of the right sizes (slabs may differ by two planes).  host_staged: through host memory (gloo)."""
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    assert len(sizes) == world and local.shape[0] == sizes[rank], (sizes, tuple(local.shape), rank)
    mine = local.contiguous()
    if local.is_cuda:
        torch.cuda.current_stream(local.device).synchronize()
    if rank != 0:
        dist.send(mine.cpu() if host_staged else mine, dst=0, group=group)
        return None
    parts = [mine]
    for r in range(1, world):
        buf = torch.empty((sizes[r],) + tuple(local.shape[1:]), dtype=local.dtype, device='cpu' if host_staged else local.device)
        dist.recv(buf, src=r, group=group)
        parts.append(buf.to(local.device))
    return torch.cat(parts, dim=0)


class LocalComm:
    """Several ranks inside ONE process (one thread per rank): used to run the distributed algorithm on a
    single GPU in tests.  Not a product path."""

    class _Shared:
        def __init__(self, world):
            self.world = world
            self.barrier = threading.Barrier(world)
            self.slots = {}

    def __init__(self, shared, rank):
        self.sh, self.rank, self.world = shared, rank, shared.world

    @staticmethod
    def make(world):
        sh = LocalComm._Shared(world)
        return [LocalComm(sh, r) for r in range(world)]

    def _sync(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.sh.barrier.wait()

    def exchange_planes(self, send_lo, send_hi, recv_lo, recv_hi):
        self.sh.slots[('lo', self.rank)] = send_lo
        self.sh.slots[('hi', self.rank)] = send_hi
        self._sync()
        if self.rank > 0:
            recv_lo.copy_(self.sh.slots[('hi', self.rank - 1)])
        if self.rank < self.world - 1:
            recv_hi.copy_(self.sh.slots[('lo', self.rank + 1)])
        self._sync()

    def all_gather(self, out, inp):
        self.sh.slots[('ag', self.rank)] = inp
        self._sync()
        n = inp.numel()
        flat = out.view(-1)
        for r in range(self.world):
            flat[r * n:(r + 1) * n].copy_(self.sh.slots[('ag', r)].view(-1))
        self._sync()


class LoopbackComm:
    """Rehearsal on ONE GPU: this rank talks to copies of itself, so a step executes every kernel and host call a
    rank of a `world`-GPU run executes, with no wire time (scripts/dist_probe.py, bench.py --rehearse-world).
    Not a product path."""

    def __init__(self, world, rank):
        self.world, self.rank = world, rank

    def exchange_planes(self, send_lo, send_hi, recv_lo, recv_hi):
        if self.rank > 0:
            recv_lo.copy_(send_hi)          # what a copy of this rank sitting below would send up
        if self.rank < self.world - 1:
            recv_hi.copy_(send_lo)

    def all_gather(self, out, inp):
        out.view(self.world, -1).copy_(inp.view(1, -1).expand(self.world, -1))


class SelfLoopDistComm(TorchDistComm):
    """Rehearsal on ONE GPU over the REAL transport: a single-rank RCCL process group in which this rank plays rank
    `rank` of `world` and both its neighbours are itself (RCCL accepts batched send/recv to self).  Same data movement as
    LoopbackComm, but through torch.distributed P2P on the side stream, so the stream / event ordering of SlabStepper is
    exercised exactly as in a multi-GPU run (tests/test_dist_slab_gpu.py, bench.py --rehearse-world W --force-dist)."""

    def __init__(self, world, rank, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        assert dist.get_world_size(group) == 1
        self.me = dist.get_rank(group)
        self.rank, self.world = rank, world
        self.bytes_sent = 0
        self.n_exchanges = 0

    def exchange_planes(self, send_lo, send_hi, recv_lo, recv_hi):
        dist, ops = self.dist, []
        if self.rank > 0:
            self.bytes_sent += send_hi.numel() * send_hi.element_size()
        if self.rank < self.world - 1:
            self.bytes_sent += send_lo.numel() * send_lo.element_size()
        # sends and receives to one peer match in order: what goes up (send_hi) must land in recv_lo, and vice versa
        if self.rank > 0 and self.rank < self.world - 1:
            ops = [dist.P2POp(dist.isend, send_hi, self.me, self.group), dist.P2POp(dist.irecv, recv_lo, self.me, self.group),
                   dist.P2POp(dist.isend, send_lo, self.me, self.group), dist.P2POp(dist.irecv, recv_hi, self.me, self.group)]
        elif self.rank > 0:
            ops = [dist.P2POp(dist.isend, send_hi, self.me, self.group), dist.P2POp(dist.irecv, recv_lo, self.me, self.group)]
        elif self.rank < self.world - 1:
            ops = [dist.P2POp(dist.isend, send_lo, self.me, self.group), dist.P2POp(dist.irecv, recv_hi, self.me, self.group)]
        if ops:
            self.n_exchanges += 1
            for r in dist.batch_isend_irecv(ops):
                r.wait()

    def all_gather(self, out, inp):
        self.bytes_sent += inp.numel() * inp.element_size() * (self.world - 1)
        one = torch.empty_like(inp)
        self.dist.all_gather_into_tensor(one, inp, group=self.group)          # the real collective, world size 1
        out.view(self.world, -1).copy_(one.view(1, -1).expand(self.world, -1))
