"""The communicators of a sharded pass -- all they offer is all_gather / all_gather_start of one small tensor per rank -- the wrapper that
counts the all-gathers passing through one, and the loop that carries a state across the ranks.  torch, torch.distributed and ctypes are
imported inside the functions: the package imports without a process group or a GPU."""
import numpy as np


class TorchDistComm:
    """all_gather over torch.distributed (backend "nccl" == RCCL over xGMI on the GPU box, "gloo" on CPU)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)

    def all_gather(self, t):
        """t: torch tensor (same shape/dtype on every rank) -> tensor [world, *t.shape] on t's device."""
        return self.all_gather_start(t)()

    def all_gather_start(self, t):
        """Enqueue the all-gather and return a function that waits for it (stream-level on GPU tensors: the host does not
        block) and returns the gathered tensor: work enqueued in between overlaps the collective."""
        import torch
        if t.is_cuda and self.dist.get_backend(self.group) == "gloo":
            # GPU tensors over a gloo group (two ranks sharing ONE GPU, which RCCL refuses: tools/two_ranks_one_gpu.sh): through the host
            torch.cuda.current_stream(t.device).synchronize()
            host = t.contiguous().cpu()
            out_h = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype)
            self.dist.all_gather_into_tensor(out_h.view(-1).view(torch.uint8), host.view(-1).view(torch.uint8), group=self.group)
            out_d = out_h.to(t.device)
            return lambda: out_d
        out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        # gathered as raw bytes: halos of uint16 captures are torch.uint16 tensors, which the nccl / gloo backends do not all take
        work = self.dist.all_gather_into_tensor(out.view(-1).view(torch.uint8), t.contiguous().view(-1).view(torch.uint8),
                                                group=self.group, async_op=True)

        def wait():
            work.wait()
            return out
        return wait


class RcclComm:
    """all_gather straight through RCCL: ncclAllGather (ctypes on the librccl.so torch itself has loaded) enqueued on the CURRENT
    torch stream with a communicator of its own -- a few microseconds of host time per exchange and no hop through a collective
    stream, against 55-80 us per torch.distributed all_gather_into_tensor (round 3, profiles/HISTORY.md: three of those per pass made
    the sharded pass host-bound).  The communicator's unique id travels through the torch.distributed group once, at start-up;
    torch.distributed is still what launches and synchronises the ranks.  `RcclComm.create(group)` falls back to TorchDistComm when
    the library or the communicator cannot be had -- on EVERY rank or on none: each step's outcome is agreed on through the group
    before the next collective step begins (`last_fallback_reason` says which step failed)."""

    _UID_BYTES = 128
    INIT_TIMEOUT_S = 120.0                 # ncclCommInitRank that has not returned by then counts as failed (the rank falls back with the others)
    last_fallback_reason = None            # why the last create() returned a TorchDistComm (None: it returned an RcclComm)

    @staticmethod
    def load_library(lib_path=None):
        """librccl.so beside torch with the five entry points this class calls, prototypes set (raises when it cannot be had)"""
        import ctypes as C
        import os
        import torch
        if lib_path is None:
            lib_path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        lib = C.CDLL(lib_path)

        class UniqueId(C.Structure):
            _fields_ = [("internal", C.c_byte * RcclComm._UID_BYTES)]
        lib.ncclGetUniqueId.restype = C.c_int
        lib.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
        lib.ncclCommInitRank.restype = C.c_int
        lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
        lib.ncclAllGather.restype = C.c_int
        lib.ncclAllGather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        lib.ncclCommDestroy.restype = C.c_int
        lib.ncclCommDestroy.argtypes = [C.c_void_p]
        lib.ncclGetErrorString.restype = C.c_char_p
        lib.ncclGetErrorString.argtypes = [C.c_int]
        lib.UniqueId = UniqueId
        return lib

    def __init__(self, group=None, lib_path=None):
        """every step on every rank succeeds or raises: use create() when a rank may fail on its own"""
        import torch
        comm, reason = self._create(group, lambda: self.load_library(lib_path), torch.device("cuda", torch.cuda.current_device()), into=self)
        if comm is None:
            raise RuntimeError(reason)

    @classmethod
    def create(cls, group=None, lib_loader=None, flag_device=None):
        """RcclComm, or TorchDistComm when RCCL cannot be reached directly (no GPU, no librccl.so beside torch, the unique id or the
        communicator could not be made, ncclCommInitRank did not return within INIT_TIMEOUT_S).  Every rank takes the same branch:
        after each step that a rank can fail on its own -- loading the library, rank 0's ncclGetUniqueId, ncclCommInitRank -- the
        ranks agree on the outcome (all_reduce MIN over the group) BEFORE any of them enters the next collective step; a rank that
        failed early therefore never leaves the others waiting in a broadcast or a communicator rendezvous.
        lib_loader / flag_device: test hooks (a stand-in library; flags on the CPU under gloo)."""
        import torch
        import torch.distributed as dist
        on_gpu = torch.cuda.is_available() and dist.get_backend(group) == "nccl"
        dev = flag_device if flag_device is not None else (torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu"))
        if lib_loader is None:
            def lib_loader():
                if not on_gpu:
                    raise RuntimeError("not an RCCL process group (no GPU, or the group's backend is not nccl)")
                return cls.load_library()
        comm, reason = cls._create(group, lib_loader, dev)
        cls.last_fallback_reason = reason
        return comm if comm is not None else TorchDistComm(group)

    @classmethod
    def _create(cls, group, lib_loader, dev, into=None):
        import ctypes as C
        import threading
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        src = dist.get_global_rank(group, 0) if group is not None else 0

        def agree(ok):
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            return int(flag.item()) == 1

        # step 1 (every rank on its own): the library and its symbols
        lib, err = None, None
        try:
            lib = lib_loader()
        except Exception as exc:                              # noqa: BLE001 -- any failure means "use torch.distributed"
            err = f"rank {rank}: librccl.so not usable: {exc!r}"
        if not agree(lib is not None):
            return None, err or "another rank could not load librccl.so"
        # step 2 (rank 0 on its own, then one broadcast every rank takes part in): the unique id, with rank 0's verdict in front
        uid = lib.UniqueId()
        ok0 = 1
        if rank == 0:
            try:
                rc = lib.ncclGetUniqueId(C.byref(uid))
                if rc != 0:
                    ok0, err = 0, f"ncclGetUniqueId: {rc}"
            except Exception as exc:                          # noqa: BLE001
                ok0, err = 0, f"ncclGetUniqueId: {exc!r}"
        t = torch.frombuffer(bytearray(bytes([ok0]) + bytes(uid)), dtype=torch.uint8).to(dev)
        dist.broadcast(t, src=src, group=group)
        raw = bytes(t.cpu().numpy().tobytes())
        if raw[0] != 1:
            return None, err or "rank 0 could not make a unique id"
        uid = lib.UniqueId.from_buffer_copy(raw[1:])
        # step 3 (a rendezvous of the ranks inside RCCL): bounded by a timeout, and agreed on afterwards
        comm = C.c_void_p()
        box = {}

        # The communicator binds to the CALLING THREAD's current device, and a new thread starts on device 0 whatever the process has
        # selected: without the set_device below every rank of a node with all GPUs visible would offer device 0 to RCCL
        # (ncclInvalidUsage, the same refusal as two ranks on one GPU -- profiles/r05_rccl_two_ranks_one_gpu.txt).
        cur_dev = torch.cuda.current_device() if torch.cuda.is_available() else None

        def init():
            try:
                if cur_dev is not None:
                    torch.cuda.set_device(cur_dev)
                box["rc"] = lib.ncclCommInitRank(C.byref(comm), world, uid, rank)
            except Exception as exc:                          # noqa: BLE001
                box["exc"] = exc
            if box.get("abandoned") and box.get("rc") == 0:   # it came up after the timeout, when every rank had fallen back: nobody will use it
                try:
                    lib.ncclCommDestroy(comm)
                except Exception:                             # noqa: BLE001
                    pass
        th = threading.Thread(target=init, daemon=True)
        th.start()
        th.join(cls.INIT_TIMEOUT_S)
        if th.is_alive():
            box["abandoned"] = True
        ok = (not th.is_alive()) and box.get("rc") == 0
        if not ok:
            err = (f"rank {rank}: ncclCommInitRank did not return within {cls.INIT_TIMEOUT_S:.0f} s" if th.is_alive() else
                   f"rank {rank}: ncclCommInitRank: {box.get('exc') or box.get('rc')}")
        self = into if into is not None else cls.__new__(cls)
        self.torch, self.C, self.lib = torch, C, lib
        self.rank, self.world = rank, world
        self.comm = comm if ok else None
        if not agree(ok):
            if ok:
                self.close()
            return None, err or "another rank could not join the communicator"
        return self, None

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.ncclGetErrorString(rc).decode()} ({rc})")

    def close(self):
        if getattr(self, "comm", None):
            self.lib.ncclCommDestroy(self.comm)
            self.comm = None

    def __repr__(self):
        return f"RcclComm(rank={self.rank}, world={self.world})"

    def _gather(self, t, stream):
        torch = self.torch
        t = t.contiguous()
        out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        nbytes = t.numel() * t.element_size()
        self._check(self.lib.ncclAllGather(t.data_ptr(), out.data_ptr(), nbytes, 1, self.comm, stream.cuda_stream), "ncclAllGather")   # 1 = ncclUint8
        return t, out

    def all_gather(self, t):
        """on the current stream, in order with the kernels around it (no event, no other stream)"""
        torch = self.torch
        with torch.cuda.device(t.device):
            keep, out = self._gather(t, torch.cuda.current_stream(t.device))
        out._urh_keep = keep                                  # the send buffer lives as long as the result
        return out

    def all_gather_start(self, t):
        """the same, as a function to call for the result (the engine-agnostic orchestration starts the halo exchange before the hot
        kernel and picks the result up after it): enqueued right here, on the current stream"""
        out = self.all_gather(t)
        return lambda: out


class _CountingComm:
    """a communicator that counts the all-gathers passing through it (ShardedPipeline._counting: `last_dc`, `last_records`, `last_auto`)"""

    def __init__(self, comm):
        self.comm, self.rank, self.world, self.count = comm, comm.rank, comm.world, 0

    def all_gather(self, t):
        self.count += 1
        return self.comm.all_gather(t)

    def all_gather_start(self, t):
        self.count += 1
        return self.comm.all_gather_start(t)


class ThreadComm:
    """W ranks as W threads of one process (lock-step through a barrier): lets a 1-GPU box (and plain CPU
    tests) execute the sharded path for any world size."""

    class Shared:
        def __init__(self, world):
            import threading
            self.world = world
            self.slots = [None] * world
            self.barrier = threading.Barrier(world)

    def __init__(self, shared, rank):
        self.shared, self.rank, self.world = shared, rank, shared.world

    def all_gather_start(self, t):
        out = self.all_gather(t)
        return lambda: out

    def all_gather(self, t):
        import torch
        sh = self.shared
        if t.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()
        sh.slots[self.rank] = t
        sh.barrier.wait()
        out = torch.stack([s.to(t.device) for s in sh.slots])
        if out.is_cuda:
            torch.cuda.current_stream(t.device).synchronize()
        sh.barrier.wait()
        return out


def carry_across_ranks(comm, gathered, compose, on_entries, hand_over):
    """Carry a state that runs through the whole capture (the Costas loop's, the sequential float32 sum's) across the ranks.
    compose(gathered, handoff) -> (entries, pending, ...): a pure function of the gathered bytes and of the exits handed over so far
    (handoff: {rank: two uint32 words}), so every rank takes the same branch -- entries[r] is rank r's true entry state or None, pending
    the first rank whose exit the gathered records cannot give (its entry is known), None when the chain holds.  on_entries(entries) is
    called after every composition; while a rank is pending, one more all-gather of hand_over(entries, pending) -- two 32-bit words per
    rank -- brings its exit.  How many all-gathers there are depends on gathered bytes only: the same on every rank.
    Returns (what the last compose returned, the number of hand-over rounds)."""
    handoff, rounds = {}, 0
    while True:
        res = compose(gathered, handoff)
        on_entries(res[0])
        if res[1] is None:
            return res, rounds
        ends = np.ascontiguousarray(comm.all_gather(hand_over(res[0], res[1])).cpu().numpy()).view(np.uint32).reshape(-1, 2)
        handoff[res[1]] = (int(ends[res[1], 0]), int(ends[res[1], 1]))
        rounds += 1
