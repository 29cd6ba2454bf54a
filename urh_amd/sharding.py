"""Sample-contiguous sharding of one long capture over the GPUs of a node.

Rank r holds samples [r*n_local, (r+1)*n_local) of the capture (the last rank may hold more or
fewer).  The hot kernel runs on every shard independently; what crosses a shard boundary is tiny and
is exchanged with three (ASK: four) small all-gathers -- no data-path collective ever moves samples:

    1. halo        the last two IQ samples of every shard (16 B)      -> seam of the FSK conj-product and
                                                                        the state of the sample before the shard
    2. summary     one ChunkInfo (72 B) per shard: the shard's run structure reduced to what its
                   neighbours need (leading run length, first / last stable run, still-short trailing run,
                   number of accepted runs)                           -> pulse-table rows with global lengths
    3. (ASK only)  first / last row of every shard's merged table     -> equal-state rows merged across shards
    4. bits        three flags per shard (long pause present, data before the first / after the last one)
                                                                      -> which boundary-spanning groups are messages

The result stays sharded: rank r owns the pulse-table rows that END in its shard and the bits /
bit_sample_pos those rows expand to; concatenating the ranks' pieces in rank order gives exactly the
single-GPU (and reference) result (`stitch`).

PSK: the Costas loop carries its state {freq, phase} across the whole capture.  A PSK pass (orders 2 and 4) first
runs the loop across the shards, then the phases above from the shard's demodulated signal:

    0. (no exchange) every rank > 0 is handed the `costas_halo_samples` raw samples before its shard (`left_raw`)
    1. speculate   candidate trajectories per 4096-sample chunk of the shard (the single-GPU kernels; chunk 0 warms
                   up in the halo), reduced to a 160-byte summary: chunk 0's candidate start states, the composition of
                   the shard's chunk maps, the last chunk's end states, "no un-gated sample"
    2. compose     all-gather the summaries; `costas_compose` (a pure function of the gathered bytes: every rank takes
                   the same branch) carries the state from {0, 1.5} across the shards by bitwise lookups.  Where it cannot,
                   the rank at the break resolves and hands its true end state over in one more all-gather of 8 bytes per
                   rank (`costas_exchange`: rounds <= world; one in the common case)
    3. resolve     every rank stitches from its true start state and writes its shard's qad
    4. halo        one all-gather of 4 bytes: every shard's last demodulated value (the seam of the pulse table), then
                   summary / rows / flags exactly as above.

Estimators: `detect_noise_level` and `detect_center` of the whole capture from the ranks' shards -- partial reductions per rank and small
all-gathers (one for the noise level; four for the center: kept counts, two records of numpy's float32 pairwise sum evaluated from the
rank's global offset, histogram counts), every result a pure function of gathered data (`pairwise_combine`, `center_parts`).  A PSK
pass detects its own center with `auto_center=True`.

Automatic passes: `iq_to_bits_auto(auto_noise=..., auto_center=...)` opens a sharded capture the way DevicePipeline.iq_to_bits(auto_noise=True,
auto_center=True) opens one on a single GPU -- the reference's defaults -- with the same bits.  auto_noise: `detect_noise_level` first (one
all-gather more), the pass gates with its value; where that is not below the sample type's max_magnitude every rank raises ValueError, decided
from the gathered value.  auto_center, PSK: as above.  auto_center, ASK and FSK -- whose fused hot kernel needs the center before the
demodulated signal exists -- take a route of their own that demodulates every shard ONCE:

    1. halo        as above (or handed over with the shard: halo_given)
    2. demodulate  the shard into the result's qad (urhgpu_shard_demod_dev: the demodulation-only kernels), and from the halo's two raw samples
                   the SEAM VALUE: the demodulated value of the sample before the shard, kept on the device
    3. center      `detect_center` of the ranks' demodulated signals (four all-gathers at most); p.center where it finds none
    4. summary / rows / flags as above, the runs segmented from the qad with that center (the qad-input kernels of the PSK pass), the seam
                   value being the left halo: the ranks do not exchange their last demodulated values

The route reads gathered values on the host and therefore refuses a pipelined engine, like PSK.  `last_auto` records the noise level, the
center, whether it was detected, and the number of all-gathers.

DC correction: `dc_correct` subtracts the mean of the WHOLE capture from every shard, bit-equal with numpy's `x - np.mean(x, axis=0)`.
Integers: one all-gather of the ranks' exact int64 column sums.  float32: the mean is the strictly sequential float32 sum of the capture,
carried across the ranks like the Costas state:

    A. sums        three 8-byte words per rank: n_local and the two column sums (float64 for float32 captures: the guesses)
    B. records     every rank speculates its shard from fl32(the float64 sum of the ranks before it) and from that guess's neighbour and
                   gathers, per column and path, {entry, exit, room}: the exit holds for every entry an even number of ulps, at most `room`,
                   from the path's (64 bytes per rank)
    C. compose     `dc_compose` (a pure function of the gathered bytes) walks the ranks with the true entry; where a record does not
                   reach, that rank re-stitches from its true entry and hands its exit over in one more all-gather of 8 bytes per rank
    D. finish      mean = fl32(double(sum) / double(n_total)); every rank subtracts it from its shard and from the raw samples handed
                   over with it (`also`)

Two all-gathers when every record holds, world + 1 at most; how many depends on gathered bytes only.

Message records: `message_records`, called on every rank after `iq_to_bits` with the same shard and the pass's result, gives one
urhgpu_msg_record per message that closes on the rank (ASK padding, first and middle position, RSSI); the ranks' arrays concatenated in rank
order (`stitch_records`) are the single-GPU records bit for bit, and `message_data` turns pieces and records into the list of
protocol.MessageData.  Only the FIRST message a rank closes can reach outside its shard (every later one starts behind a pause row that ends
in the shard and is closed by a pause that ends in it), so what crosses the ranks is small:

    1. summary     ten 8-byte words per rank (REC_* below; include/urhgpu.h): pos_base, n_local, messages closed, bits / position entries
                   before the first and behind the last close, the first closed message's pause, "capacities held", position entries
                   -> `records_plan`: L, np, n_pad, the middle index of every rank's first message and who holds its entries 0 and rel
    2. look-up     2 x world position entries, every rank fills in the ones it holds -> first_pos, mid_pos and the window of every first message
    3. windows     only if a first window is not wholly inside its closing rank's shard: the raw samples of those windows, every rank the part
                   its shard holds; the closing rank assembles its window contiguously

Two all-gathers in the common case, three at most, none for one rank; which, depends on gathered words only.

The orchestration below is engine-agnostic: `engine` is the GPU engine (urh_amd.shard_engine.GpuShardEngine,
HIP kernels behind the C ABI) in production; the CPU test-suite drives the same orchestration with the executable
model of the kernels (tests/model_shard.py) over a world_size-2 gloo group.
"""
import contextlib

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
    """a communicator that counts the all-gathers passing through it (iq_to_bits_auto: `last_auto`)"""

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


COSTAS_SUMMARY_BYTES = 160                  # URHGPU_COSTAS_SUMMARY_BYTES
COSTAS_START = (0x00000000, 0x3FC00000)     # the loop's initial state {freq 0.0f, phase 1.5f} as float32 bits (signal_functions.pyx:261)
_COSTAS_WARM_BACK = 16                      # kWarmBackFactor (costas.hip): a candidate looks back at most 16 x its warm-up


def costas_halo_samples(bandwidth, pos_base=None):
    """urhgpu_costas_halo_samples: raw samples before its shard that a PSK rank > 0 is handed (`left_raw`) -- every sample the
    warm-up of its first chunk may read: 8 192 at bandwidth 0.1, up to 131 072 at the smallest bandwidths.  pos_base given: no more
    than the capture holds before the shard from sample 1 on (sample 0 is not part of the loop)."""
    want = 40.0 / max(1e-3, min(1.0, abs(float(np.float32(bandwidth)))))      # costas_warm (costas.hip), in double
    w = 256
    while w < want and w < 8192:
        w *= 2
    h = _COSTAS_WARM_BACK * w
    return h if pos_base is None else min(h, max(int(pos_base) - 1, 0))


def pack_costas_summary(starts, ends, cmap, reps, identity=False, n_chunks=1, ungated=None):
    """One Costas shard summary in the layout k_costas_shard_summary (costas.hip) writes: uint8 (COSTAS_SUMMARY_BYTES,).
    starts / ends: K states (freq bits, phase bits) of the first chunk's candidates / the last chunk's (None: not a representative);
    cmap: the composed chunk map (nibble k: last-chunk candidate of first-chunk candidate k, 0xF broken); reps: K flags."""
    w = np.zeros(COSTAS_SUMMARY_BYTES // 4, np.uint32)
    for k, s in enumerate(starts):
        w[2 * k], w[2 * k + 1] = s
    for k, e in enumerate(ends):
        if e is not None:
            w[16 + 2 * k], w[17 + 2 * k] = e
    w[32] = cmap
    w[33] = sum(1 << k for k, r in enumerate(reps) if r)
    w[34] = 1 if identity else 0
    w[35] = len(starts)
    w[36:38] = np.array([n_chunks], np.int64).view(np.uint32)
    w[38:40] = np.array([(0 if identity else 1) if ungated is None else ungated], np.int64).view(np.uint32)
    return w.view(np.uint8)


def costas_compose(summaries, handoff=None):
    """Carry the Costas loop state across the shards: a pure function of the gathered summaries ((world, COSTAS_SUMMARY_BYTES)
    bytes, rank order) and of the end states handed over so far (handoff: {rank: (freq bits, phase bits)}), so every rank that
    evaluates it takes the same branch.  Rank 0 starts in COSTAS_START; a shard without an un-gated sample passes the state on;
    otherwise the state is looked up BITWISE among the representatives of its first chunk's candidates and the composed map names
    the last-chunk candidate whose end state comes out.  Returns (starts, pending): starts[r] = the true state at the start of shard
    r as (freq bits, phase bits), None where not known yet; pending = the first rank whose end state the summaries cannot give (its
    start state is known: it resolves and hands its end state over), None when every start state is known."""
    raw = np.ascontiguousarray(np.asarray(summaries, dtype=np.uint8)).reshape(-1, COSTAS_SUMMARY_BYTES)
    w = raw.view("<u4")
    handoff = handoff or {}
    starts = [None] * len(w)
    state = COSTAS_START
    for r, row in enumerate(w):
        starts[r] = state
        if r in handoff:
            state = (int(handoff[r][0]), int(handoff[r][1]))
            continue
        if row[34]:
            continue                                  # gated samples freeze the loop: end state = start state
        K, reps, cmap = int(row[35]), int(row[33]), int(row[32])
        q = 0xF
        for k in range(min(K, 8)):
            if (reps >> k) & 1 and (int(row[2 * k]), int(row[2 * k + 1])) == state:
                q = (cmap >> (4 * k)) & 0xF
                break
        if q >= min(K, 8):                            # no candidate starts in the state, or the map is broken
            return starts, r
        state = (int(row[16 + 2 * q]), int(row[17 + 2 * q]))
    return starts, None


def costas_exchange(comm, summary, resolve, end_state):
    """Steps 2-3 of a PSK pass (module docstring): all-gather the summaries, compose, and let this rank resolve as soon as its start
    state is known; while the chain breaks at some rank, that rank's end state comes in one more all-gather.  How many all-gathers
    there are depends on the gathered bytes only (costas_compose): the same on every rank.
    summary: this rank's summary (uint8 tensor); resolve((freq bits, phase bits)) stitches this rank from its true start state;
    end_state(): 2 x int32 tensor, the rank's true end state once it has resolved.  Returns the number of rounds."""
    summaries = comm.all_gather(summary).cpu().numpy()
    handoff = {}
    rounds, resolved = 1, False
    while True:
        starts, pending = costas_compose(summaries, handoff)
        if not resolved and starts[comm.rank] is not None:
            resolve(starts[comm.rank])
            resolved = True
        if pending is None:
            return rounds
        ends = np.ascontiguousarray(comm.all_gather(end_state()).cpu().numpy()).view(np.uint32).reshape(-1, 2)
        handoff[pending] = (int(ends[pending, 0]), int(ends[pending, 1]))
        rounds += 1


# ---- the sequential float32 sum of a capture across ranks (csrc/dc_correct.hip writes the records) -------------------------------------
# a rank's records: [column][path] x {entry bits, exit bits, room, flags} as uint32 (URHGPU_DC_RECORD_BYTES = 64)
DC_IDENTITY = 1                             # flags: the shard holds no sample, its exit is its entry


def dc_compose(records, handoff=None):
    """Carry numpy's sequential float32 column sums across the shards: a pure function of the gathered shard records ((world, 2, 2, 4)
    uint32: per column and speculated path {entry bits, exit bits, room, flags}, rank order) and of the exits handed over so far
    (handoff: {rank: (bits I, bits Q)}), so every rank that evaluates it takes the same branch.  Rank 0 enters with +0.0.  A shard's
    exit follows from its records where the true entry equals a path's entry (the recorded exit), where it lies D ulps from the path an
    even number of ulps away, on the same side of zero, with |D| <= room (the recorded exit moved by D: every chunk on the path stays
    inside its binade, and paths an even distance apart round every tie alike), where the shard is empty, and where the sum is already
    NaN (it stays).  Returns (entries, pending, total): entries[r] = the true entry of shard r as (bits I, bits Q), None where not known
    yet; pending = the first rank one of whose columns the records cannot carry (its entry is known: it re-stitches both columns from
    it and hands its exits over), None when every entry is known; total = the sum's bits (I, Q) when pending is None."""
    rec = np.ascontiguousarray(np.asarray(records)).view(np.uint32).reshape(-1, 2, 2, 4)
    handoff = handoff or {}
    entries = [None] * len(rec)
    t = (0, 0)                                            # +0.0: numpy's accumulator starts there
    for r in range(len(rec)):
        entries[r] = t
        if r in handoff:
            t = (int(handoff[r][0]), int(handoff[r][1]))
            continue
        nxt = []
        for col in range(2):
            e = _dc_exit(rec[r, col], t[col])
            if e is None:
                return entries, r, None
            nxt.append(e)
        t = tuple(nxt)
    return entries, None, t


def _dc_exit(paths, t):
    """the exit of one column of a shard entered with the bits t, from its two path records; None where they do not give it"""
    if int(paths[0, 3]) & DC_IDENTITY:
        return t
    for p in paths:
        if t == int(p[0]):
            return int(p[1])
    if (t & 0x7FFFFFFF) > 0x7F800000:
        return t                                          # a NaN sum absorbs whatever follows
    p = paths[(t ^ int(paths[0, 0])) & 1]                 # the path an even number of ulps away
    entry, leave, room = int(p[0]), int(p[1]), int(p[2])
    if (t ^ entry) >> 31:
        return None
    d = (t & 0x7FFFFFFF) - (entry & 0x7FFFFFFF)
    if abs(d) > room:
        return None
    return (leave & 0x80000000) | ((leave & 0x7FFFFFFF) + d)


# ---- numpy's float32 summation tree across ranks (csrc/pairwise.hpp has the order; csrc/shard_estimators.hip writes the records) ----
PW_PIECE, PW_LEAF = 8192, 128               # kPwChunk, kPwLeaf
PW_REC_HEAD, PW_REC_FIRST, PW_REC_LAST, PW_REC_TAIL, PW_REC_PIECES = 8, 136, 264, 392, 520      # URHGPU_PW_REC_* (include/urhgpu.h)
HIST_GATHER_BINS = 1 << 22                  # bins per all-gather of detect_center's histogram (32 MiB of int64 per rank)


def pairwise_inside_pieces(g_off: int, m_local: int, m_total: int):
    """[pa, pb): the full pieces of PW_PIECE elements that lie wholly inside [g_off, g_off + m_local) of a sequence of m_total"""
    pa = -(-g_off // PW_PIECE)
    pb = min((g_off + m_local) // PW_PIECE, m_total // PW_PIECE)
    return pa, max(pa, pb)


def pairwise_record_words(g_off: int, m_local: int, m_total: int) -> int:
    """length in float32 words of the record urhgpu_pairwise_partial_f32_dev writes for that range"""
    pa, pb = pairwise_inside_pieces(g_off, m_local, m_total)
    return PW_REC_PIECES + pb - pa


def pairwise_piece_leaves(p: int, m_total: int):
    """the leaves of piece p as (offset in the piece, length): 64 leaves of 128 for a full piece, pw's recursive split (the left part
    is n // 2 rounded down to a multiple of 8) for the irregular last one"""
    if p < m_total // PW_PIECE:
        return [(k * PW_LEAF, PW_LEAF) for k in range(PW_PIECE // PW_LEAF)]
    out = []

    def split(off, n):
        if n <= PW_LEAF:
            out.append((off, n))
            return
        n2 = n // 2
        n2 -= n2 % 8
        split(off, n2)
        split(off + n2, n - n2)
    split(0, m_total % PW_PIECE)
    return out


def pairwise_leaf_sum(a) -> np.float32:
    """pw over one leaf (len(a) <= PW_LEAF) in float32, as pw_leaf (csrc/pairwise.hpp): 8 strided accumulators, their fixed tree, the
    len % 8 tail in order; fewer than 8 elements: in order from 0"""
    a = np.asarray(a, dtype=np.float32)
    n = len(a)
    with np.errstate(all="ignore"):
        if n < 8:
            res = np.float32(0.0)
            for v in a:
                res = np.float32(res + v)
            return res
        nb = n - n % 8
        r = np.add.accumulate(a[:nb].reshape(-1, 8), axis=0, dtype=np.float32)[-1]       # r[j] += a[i + j], row after row
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) +
                         np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in a[nb:]:
            res = np.float32(res + v)
        return res


def pairwise_tree(leaf_sums, lengths) -> np.float32:
    """pw's additions above the leaves: leaf_sums[i] is the sum of a leaf of lengths[i] elements, in order"""
    vals = [np.float32(v) for v in leaf_sums]
    pos = 0

    def node(n):
        nonlocal pos
        if n <= PW_LEAF:
            v = vals[pos]
            pos += 1
            return v
        n2 = n // 2
        n2 -= n2 % 8
        left = node(n2)
        right = node(n - n2)
        return np.float32(left + right)
    with np.errstate(all="ignore"):
        return node(int(sum(lengths)))


def _record_headers(records):
    recs = np.ascontiguousarray(records, dtype=np.float32)
    recs = recs.reshape(len(recs), -1)
    hdr = np.ascontiguousarray(recs[:, 0:4]).view(np.int64)
    return recs, [int(v) for v in hdr[:, 0]], [int(v) for v in hdr[:, 1]]


def pairwise_combine(records, m_total: int) -> np.float32:
    """np.add.reduce of a float32 sequence of m_total elements from the ranks' records (urhgpu_pairwise_partial_f32_dev; rank order,
    rows padded to one length): a pure function of its arguments, so every rank that evaluates it gets the same bits.  Leaves that
    a shard boundary cuts are finished from the ranks' raw elements with pw_leaf's arithmetic, pieces that one cuts from their leaf
    sums, and the pieces are accumulated left to right -- all in float32 (numpy float32 scalars: no excess precision)."""
    recs, g_offs, m_locals = _record_headers(records)
    m_total = int(m_total)
    if m_total <= 0:
        return np.float32(0.0)
    ranks = [r for r in range(len(recs)) if m_locals[r] > 0]
    at = 0
    for r in ranks:
        if g_offs[r] != at:
            raise ValueError("pairwise_combine: the ranks' ranges do not tile the sequence")
        at += m_locals[r]
    if at != m_total:
        raise ValueError("pairwise_combine: the ranks' ranges do not tile the sequence")
    n_pieces = -(-m_total // PW_PIECE)
    sums = np.zeros(n_pieces + 1, dtype=np.float32)          # sums[0]: the 0 np.add.reduce starts from
    have = np.zeros(n_pieces, dtype=bool)
    for r in ranks:
        pa, pb = pairwise_inside_pieces(g_offs[r], m_locals[r], m_total)
        sums[1 + pa:1 + pb] = recs[r, PW_REC_PIECES:PW_REC_PIECES + pb - pa]
        have[pa:pb] = True
    ends = np.array([g_offs[r] + m_locals[r] for r in ranks], dtype=np.int64)
    for p in np.nonzero(~have)[0].tolist():
        leaves = pairwise_piece_leaves(p, m_total)
        vals = []
        for off, ln in leaves:
            l0, l1 = p * PW_PIECE + off, p * PW_PIECE + off + ln
            k = int(np.searchsorted(ends, l0, side="right"))      # the rank that holds element l0
            r = ranks[k]
            if ends[k] >= l1:                                      # the leaf lies wholly inside that rank
                area = PW_REC_FIRST if p == g_offs[r] // PW_PIECE else PW_REC_LAST
                vals.append(recs[r, area + (off + 63) // 64])
                continue
            raw = []
            while k < len(ranks) and g_offs[ranks[k]] < l1:
                r = ranks[k]
                lo, hi = max(l0, g_offs[r]), min(l1, int(ends[k]))
                src = PW_REC_HEAD if l0 < g_offs[r] else PW_REC_TAIL
                raw.append(recs[r, src:src + hi - lo])
                k += 1
            vals.append(pairwise_leaf_sum(np.concatenate(raw)))
        sums[1 + p] = pairwise_tree(vals, [ln for _, ln in leaves])
    with np.errstate(all="ignore"):
        return np.add.accumulate(sums, dtype=np.float32)[-1]      # ((0 + piece 0) + piece 1) + ...: left to right


def minmax_combine(records):
    """util.minmax (util.pyx:20-36) of the whole sequence from the records' words 4-6: seeded with the sequence's first element, a NaN
    never replaces a value -- so a NaN first element stays, and any other is ignored.  Returns (min, max) as floats, None when every
    rank is empty."""
    recs, _, m_locals = _record_headers(records)
    ranks = [r for r in range(len(recs)) if m_locals[r] > 0]
    if not ranks:
        return None
    mn = mx = recs[ranks[0], 6]
    for r in ranks:
        if recs[r, 4] < mn:
            mn = recs[r, 4]
        if recs[r, 5] > mx:
            mx = recs[r, 5]
    return float(mn), float(mx)


def center_parts(kept_counts, max_size=None):
    """detect_center's trimmed sequence S = R[int(0.05 K) : int(0.95 K)] (cut to max_size) of the ranks' kept samples R, from the gathered
    kept counts: (m, [(local begin, g_r, m_r) per rank]) -- rank r's part of S is kept_r[begin : begin + m_r], elements [g_r, g_r + m_r) of
    S (m_r may be 0).  A pure function of the gathered counts."""
    counts = [int(v) for v in kept_counts]
    total = sum(counts)
    a, b = int(0.05 * total), int(0.95 * total)                    # AutoInterpretation.py:231
    m = b - a
    if max_size is not None and m > max_size:                      # :233-234
        m = int(max_size)
    parts, c0 = [], 0
    for k in counts:
        lo, hi = max(c0, a), min(c0 + k, a + m)
        if hi > lo:
            parts.append((lo - c0, lo - a, hi - lo))
        else:
            parts.append((0, min(max(c0 - a, 0), m), 0))
        c0 += k
    return m, parts


# ---- message records across ranks (csrc/msg_records.hip: k_shard_rec_summary writes the words, k_shard_msg_records takes the descriptor) ----
REC_SUMMARY_WORDS = 10                      # URHGPU_SHARD_REC_SUMMARY_WORDS
(REC_POS_BASE, REC_N_LOCAL, REC_N_MSG, REC_HEAD_BITS, REC_HEAD_POS, REC_TAIL_BITS, REC_TAIL_POS, REC_FIRST_PAUSE, REC_HELD, REC_N_POS) = range(10)
REC_FIRST_WORDS = 8                         # URHGPU_SHARD_REC_FIRST_WORDS: {closes, L, np, n_pad, first_pos, mid_pos, ok, window assembled}


def records_plan(words, n_total, samples_per_symbol, divisor):
    """The first message of every closing rank from the gathered summary words ((world, REC_SUMMARY_WORDS) int64, rank order): a pure
    function of its arguments, so every rank that evaluates it takes the same branch.  Raises ValueError where the shards do not tile
    [0, n_total).  divisor: message_length_divisor for an ASK pass, 1 otherwise.  Returns a list with one entry per rank: None where the
    rank closes no message, else dict(L, np, pause, n_pad, k, rel, add, ok, first, mid) -- L bits and np position entries summed over the
    ranks since the previous close, the padding decision and the middle index as k_msg_records takes them (rel = np - 2 and
    add = (k - rel) * sps where the middle lies in the padded part, rel = k and add = 0 otherwise), first / mid = (rank, local index) of the
    position entries 0 and rel; ok False (first / mid None) where a contributing rank exceeded a capacity or the entries do not exist."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.int64).reshape(-1, REC_SUMMARY_WORDS)
    sps, divisor = int(samples_per_symbol), int(divisor)
    at = 0
    for row in w:
        if int(row[REC_POS_BASE]) != at or int(row[REC_N_LOCAL]) < 0:
            raise ValueError("message_records: the ranks' shards do not tile the capture")
        at += int(row[REC_N_LOCAL])
    if at != int(n_total):
        raise ValueError(f"message_records: the ranks hold {at} samples, the capture has {int(n_total)}")
    plan, prev = [None] * len(w), -1
    for r, row in enumerate(w):
        if int(row[REC_N_MSG]) <= 0:
            continue
        # the ranks that contribute, in order: (rank, local index of its first entry, entries, bits)
        parts = []
        if prev >= 0:
            parts.append((prev, int(w[prev, REC_N_POS] - w[prev, REC_TAIL_POS]), int(w[prev, REC_TAIL_POS]), int(w[prev, REC_TAIL_BITS])))
        parts += [(q, 0, int(w[q, REC_HEAD_POS]), int(w[q, REC_HEAD_BITS])) for q in range(prev + 1, r + 1)]
        held = all(int(w[q, REC_HELD]) == 1 for q, _, _, _ in parts)
        L, n_pos, pause = sum(b for _, _, _, b in parts), sum(c for _, _, c, _ in parts), int(row[REC_FIRST_PAUSE])
        n_pad = 0
        if divisor > 1 and L >= 0:
            missing = (divisor - L % divisor) % divisor
            if missing > 0 and pause >= sps * missing:
                n_pad = missing
        k = (L + n_pad) // 2
        in_pad = n_pad > 0 and k > n_pos - 2
        rel = n_pos - 2 if in_pad else k
        ok = held and L >= 0 and n_pos >= 1 and 0 <= rel < n_pos and all(c >= 0 and a >= 0 for _, a, c, _ in parts)

        def locate(e):
            for q, a, c, _ in parts:
                if e < c:
                    return q, a + e
                e -= c
        plan[r] = dict(L=L, np=n_pos, pause=pause, n_pad=n_pad, k=k, rel=rel, add=(k - rel) * sps if in_pad else 0, ok=ok,
                       first=locate(0) if ok else None, mid=locate(rel) if ok else None)
        prev = r
    return plan


def records_requests(plan, rank):
    """the look-up a rank answers: int64 (2 * world,), slot 2r / 2r + 1 = the LOCAL index of entry 0 / rel of rank r's first message where
    `rank` holds it, -1 elsewhere"""
    idx = np.full(2 * len(plan), -1, np.int64)
    for r, m in enumerate(plan):
        if m is not None and m["ok"]:
            for slot, (q, at) in ((2 * r, m["first"]), (2 * r + 1, m["mid"])):
                if q == rank:
                    idx[slot] = at
    return idx


def _py_slice(start, stop, n):
    """Python's a[start:stop] on n elements: (where the slice begins, how many elements it has)"""
    a = max(start + n, 0) if start < 0 else min(start, n)
    b = max(stop + n, 0) if stop < 0 else min(stop, n)
    return a, max(b - a, 0)


def records_windows(plan, words, values, n_total, samples_per_symbol):
    """first_pos, mid_pos and the window of every first message from the plan and the gathered look-up ((world, 2 * world) int64): a pure
    function of gathered data.  Returns (firsts, outside): firsts[r] = None or dict(first_pos, mid_pos, lo, w, slot) -- the window is
    samples [lo, lo + w) of the capture, clipped at the CAPTURE's end, slot = its index among the exchanged windows or -1 where it lies
    wholly inside rank r's shard (or is empty); outside = the closing ranks whose window is exchanged, in order."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.int64).reshape(-1, REC_SUMMARY_WORDS)
    v = np.ascontiguousarray(np.asarray(values)).view(np.int64).reshape(len(w), 2 * len(w))
    firsts, outside = [None] * len(w), []
    for r, m in enumerate(plan):
        if m is None or not m["ok"]:
            continue
        first_pos = int(v[m["first"][0], 2 * r])
        mid_pos = int(v[m["mid"][0], 2 * r + 1]) + m["add"]
        lo, cnt = _py_slice(mid_pos, mid_pos + int(samples_per_symbol), int(n_total))
        a, b = int(w[r, REC_POS_BASE]), int(w[r, REC_POS_BASE] + w[r, REC_N_LOCAL])
        slot = -1
        if cnt > 0 and not (a <= lo and lo + cnt <= b):
            slot = len(outside)
            outside.append(r)
        firsts[r] = dict(first_pos=first_pos, mid_pos=mid_pos, lo=lo, w=cnt, slot=slot)
    return firsts, outside


def shard_bounds(n_total: int, world: int):
    """[begin, end) of every rank's shard: equal shards of ceil(n/world) samples rounded up to a multiple of
    64 (so that every shard starts 16-byte aligned for every IQ dtype), the last rank takes what is left.
    Every shard needs >= 2 samples."""
    per = -(-n_total // world)
    per = -(-per // 64) * 64
    b = [min(r * per, n_total) for r in range(world + 1)]
    b[world] = n_total
    if any(b[r + 1] - b[r] < 2 for r in range(world)):
        raise ValueError(f"capture of {n_total} samples is too short to shard over {world} ranks")
    return [(b[r], b[r + 1]) for r in range(world)]


class ShardedPipeline:
    """One rank's view of the sharded IQ->bits pass."""

    def __init__(self, engine, comm):
        self.engine, self.comm = engine, comm
        self.rank, self.world = comm.rank, comm.world
        self.last_costas = None                  # PSK: the last pass's Costas exchange (rounds, this rank's chunks by map / checkpoint / serial)
        self.last_center = None                  # the center the last pass's pulse table was built with (auto_center: the detected one)
        self.last_dc = None                      # the last dc_correct: mean, all-gathers, this rank's stitch statistics
        self.last_records = None                 # the last message_records: all-gathers, windows exchanged
        self.last_auto = None                    # the last iq_to_bits_auto: noise, center, center_detected, all_gathers
        self._center_found = False               # the last pass's pulse table was built with a center it detected

    # bench.py / DevicePipeline compatible surface ------------------------------------------------
    @property
    def ctx(self):
        return self.engine.ctx

    def reserve(self, n_local, p):
        self.engine.reserve(n_local, p)

    def fir_filter(self, iq_local, taps, left_raw=None, want_halo=False, raw_halo=None):
        """Signal.filter_range semantics on a sharded capture (BASELINE.json configs[3], "FIR-halo exchange"): every rank
        filters its shard with the m-1 samples that precede it as history; rank 0 starts from zero history like the
        reference's fir_filter (signal_functions.pyx:513-525).  Returns the filtered shard (same shape as iq_local).
        left_raw is None: the history is the left neighbour's tail, one all-gather of (m-1) * 8 bytes per rank.
        left_raw given (every rank but the first; round 5): whoever distributed the capture handed the rank the m + 1 RAW samples
        that precede its shard ((m + 1, 2) float32 / complex64 (m + 1,): 520 bytes for 64 taps) -- no exchange at all: the last
        m - 1 of them are the filter's history, and filtering the m + 1 themselves gives, in their last two outputs, the two FILTERED
        samples before the shard, i.e. the demodulation's halo (want_halo=True: returns (filtered shard, that halo or None)).
        raw_halo states the mode and must be THE SAME ON EVERY RANK (a rank that guessed it from its own arguments could skip a
        collective the others enter): True = raw mode (rank 0 passes no left_raw, every other rank must), False = exchange,
        None = raw mode iff want_halo (the halo only exists in raw mode; left_raw without want_halo also selects it on ranks > 0,
        where rank 0 then has to say raw_halo=True)."""
        e, c = self.engine, self.comm
        if raw_halo is None:
            raw_halo = bool(want_halo) or left_raw is not None
        m = int(taps.shape[0])                     # complex64 (m,) or float32 (m, 2): rows = taps
        if m <= 1 or self.world == 1:
            out = e.fir(iq_local, taps, None)
            return (out, None) if want_halo else out
        if int(iq_local.shape[0]) < m - 1:
            raise ValueError("shard shorter than the filter history")
        if want_halo and not raw_halo:
            raise ValueError("want_halo needs raw_halo: the filtered halo comes from the raw samples handed over with the shard")
        if raw_halo:
            if self.rank == 0:
                out = e.fir(iq_local, taps, None)
                return (out, None) if want_halo else out
            if left_raw is None:
                raise ValueError("raw_halo: ranks > 0 pass the m + 1 raw samples that precede their shard as left_raw")
            raw = left_raw
            if hasattr(e, "torch") and raw.dtype == e.torch.complex64:
                raw = e.torch.view_as_real(raw)
            if int(raw.shape[0]) != m + 1:
                raise ValueError("left_raw: the m + 1 raw samples that precede the shard")
            out = e.fir(iq_local, taps, raw[2:].contiguous())
            if not want_halo:
                return out
            return out, e.fir(raw.contiguous(), taps, None)[-2:].contiguous()     # outputs m - 1 and m have their full history inside `raw`
        tails = c.all_gather(e.fir_tail(iq_local, m - 1))
        return e.fir(iq_local, taps, tails[self.rank - 1] if self.rank > 0 else None)

    # the estimators that feed the pipelines: partial reductions per rank + small all-gathers -------------------
    def _estimator_engine(self, *names):
        missing = [n for n in names if not hasattr(self.engine, n)]
        if missing:
            raise NotImplementedError(f"the engine offers no {', '.join(missing)}")
        return self.engine

    def detect_noise_level(self, iq_local, pos_base=None, n_total=None):
        """AutoInterpretation.detect_noise_level(get_magnitudes(capture)) (AutoInterpretation.py:60-91) for the capture whose shard
        [pos_base, pos_base + n_local) this rank holds; pos_base / n_total default as in iq_to_bits.  The chunk geometry is the
        capture's (estimators.noise_chunks(n_total): chunks counted from the end, the front remainder dropped): a chunk may straddle
        any number of shards.  Every rank reduces the intersection of every chunk with its shard to an fp64 sum and a max
        (urhgpu_magnitude_chunk_partials_dev), ONE all-gather moves 2 * n_chunks doubles per rank, and every rank adds the sums in
        rank order and folds the maxima (a NaN stays) before the decision of the single-GPU function.  A capture of three samples or
        fewer gives 0 without a collective; on one rank the value is detect_noise_level_dev's.
        The sums are fp64 sums in another order than numpy's pairwise one ("detect_noise_level"): the float32-cast chunk
        means agree with numpy's unless an fp64 sum lies within an ulp of a float32 rounding boundary."""
        from .estimators import noise_chunks, noise_level_from_chunk_stats
        e, c = self._estimator_engine("noise_partials"), self.comm
        n_local = int(iq_local.shape[0])
        pos_base = self.rank * n_local if pos_base is None else int(pos_base)
        n_total = self.world * n_local if n_total is None else int(n_total)
        if pos_base < 0 or pos_base + n_local > n_total:
            raise ValueError("detect_noise_level: the shard does not lie inside the capture")
        chunk, n_chunks = noise_chunks(n_total) if n_total > 3 else (1, 0)
        part = e.noise_partials(iq_local, pos_base, n_total, chunk, n_chunks)     # checks the shard before anything is exchanged
        if n_total <= 3:                                                          # :61-62
            return 0
        both = np.asarray(c.all_gather(part).cpu().numpy(), dtype=np.float64).reshape(self.world, 2, n_chunks)
        sums = np.zeros(n_chunks, np.float64)
        for r in range(self.world):
            sums = sums + both[r, 0]
        maxs = both[:, 1].max(axis=0)                                             # np.max: a NaN stays, as within a rank
        return noise_level_from_chunk_stats(sums, maxs, chunk)

    def detect_center(self, qad_local, max_size=None):
        """AutoInterpretation.detect_center(qad, max_size) (AutoInterpretation.py:226-277) where qad is the concatenation of the ranks'
        qad_local (float32, 1-D, on the rank's device) in rank order: bit-equal to estimators.detect_center_dev on the whole signal,
        None on every rank where that gives None.  max_size must be the same on every rank.  Four all-gathers at most:
            1. the kept counts of the local compaction qad > -4 -> the trim [int(0.05 K), int(0.95 K)) and every rank's part of it
            2. the records of np.mean's float32 sum (urhgpu_pairwise_partial_f32_dev, which also takes min / max in that pass)
            3. the records of np.var's second sum, (x - mean)^2 in float32
            4. the int64 counts of np.histogram over the edges every rank computes from the same scalars (more than HIST_GATHER_BINS
               bins -- a nearly constant signal -- go in blocks of that many)
        The sums are numpy's float32 pairwise sums bit for bit (pairwise_combine finishes what the shard boundaries cut).  Every
        early return is decided from gathered data."""
        from .estimators import peaks_center
        e, c = self._estimator_engine("compact_gt", "pairwise_partial", "histogram"), self.comm
        if max_size is not None and int(max_size) < 0:
            raise ValueError("detect_center: max_size must not be negative")
        kept, cnt = e.compact_gt(qad_local, -4.0)                                 # checks the shard before anything is exchanged
        counts = c.all_gather(cnt).cpu().numpy().reshape(-1)
        m, parts = center_parts(counts, max_size)
        if m == 0:
            return None             # np.var of an empty slice is nan -> np.arange raises ValueError -> None (:246-248)
        begin, g_r, m_r = parts[self.rank]
        mine = kept[begin:begin + m_r]
        words = max(pairwise_record_words(g, k, m) for _, g, k in parts)
        recs = c.all_gather(e.pairwise_partial(mine, g_r, m, 0, 0.0, words)).cpu().numpy()
        hist_min, hist_max = minmax_combine(recs)
        with np.errstate(all="ignore"):
            mean = pairwise_combine(recs, m) / np.float32(m)                      # np.mean: float32 sum / float32 count
            recs = c.all_gather(e.pairwise_partial(mine, g_r, m, 1, float(mean), words)).cpu().numpy()
            hist_step = float(pairwise_combine(recs, m) / np.float32(m))          # float(np.var(rect)) (:240)
        try:
            with np.errstate(all="ignore"):
                edges = np.arange(hist_min, hist_max + hist_step, hist_step)      # :243-245
            if len(edges) < 2:
                return None         # np.histogram with fewer than 2 edges raises ValueError -> None (:246-248)
        except (ZeroDivisionError, ValueError):
            return None
        local = e.histogram(mine, edges)
        n_bins = len(edges) - 1
        total = np.zeros(n_bins, np.int64)
        for b0 in range(0, n_bins, HIST_GATHER_BINS):
            b1 = min(n_bins, b0 + HIST_GATHER_BINS)
            total[b0:b1] = c.all_gather(local[b0:b1]).cpu().numpy().reshape(self.world, -1).sum(axis=0)
        return peaks_center(total, edges)

    def dc_correct(self, iq_local, pos_base=None, n_total=None, also=(), out=None):
        """The shard minus the mean of the WHOLE capture: rows [pos_base, pos_base + n_local) of numpy's x - np.mean(x, axis=0) stored into the
        capture's sample type, bit for bit -- the sharded counterpart of filter.dc_correct_dev (module docstring, "DC correction").
        iq_local: (n_local, 2) in one of the five sample types, or complex64 (n_local,); a rank may hold no sample.  pos_base / n_total
        default as in iq_to_bits; the ranks' n_local must add up to n_total (checked from gathered data: every rank raises ValueError).
        also: small tensors of the same sample type corrected with the same mean and returned with the shard -- the raw samples a
        distributor hands over with it (left_halo, the PSK left_raw, the FIR left_raw), without which a corrected shard could not be
        used with halo_given=True, a PSK pass or fir_filter(raw_halo=True).  out: None (a new tensor) or iq_local (in place).
        Returns the corrected shard, or (shard, [corrected also tensors]) when `also` is given.  `last_dc` records the mean (two float64
        for integers, two float32 for float32), the number of all-gathers and this rank's stitch statistics.
        world == 1 is the single-GPU function; n_total == 0 returns the empty shard; neither enters a collective.  The recipe for a
        corrected pass: dc_correct, then iq_to_bits on the result."""
        e = self._estimator_engine("dc_own", "dc_whole", "dc_sums", "dc_spec", "dc_resolve", "dc_apply", "dc_stats")
        c = self.comm
        also = tuple(also)
        is_f32 = e.dc_own(iq_local, also, out)            # everything a rank can get wrong on its own, before anything is exchanged
        n_local = int(iq_local.shape[0])
        pos_base = self.rank * n_local if pos_base is None else int(pos_base)
        n_total = self.world * n_local if n_total is None else int(n_total)
        if pos_base < 0 or pos_base + n_local > n_total:
            raise ValueError("dc_correct: the shard does not lie inside the capture")
        stats = {"chunks": 0, "derived": 0, "reevaluated": 0}
        gathers = 0
        if self.world == 1 and n_local != n_total:
            raise ValueError(f"dc_correct: the ranks hold {n_local} samples, the capture has {n_total}")
        if n_total == 0:
            self.last_dc = {"mean": None, "all_gathers": 0, **stats}
            return (iq_local, list(also)) if also else iq_local
        if self.world == 1:
            res, mean = e.dc_whole(iq_local, out)
            stats = e.dc_stats()
        else:
            words = np.ascontiguousarray(c.all_gather(e.dc_sums(iq_local)).cpu().numpy()).view(np.int64).reshape(self.world, 3)
            gathers = 1
            held = sum(int(v) for v in words[:, 0])
            if held != n_total:                           # decided from gathered data: every rank raises, none is left in a collective
                raise ValueError(f"dc_correct: the ranks hold {held} samples, the capture has {n_total}")
            if not is_f32:
                mean = np.array([float(sum(int(v) for v in words[:, k])) / float(n_total) for k in (1, 2)], np.float64)
            else:
                with np.errstate(all="ignore"):
                    guesses = np.ascontiguousarray(words[:, 1:]).view(np.float64)
                    base = [0.0, 0.0]
                    for r in range(self.rank):
                        base = [base[0] + float(guesses[r, 0]), base[1] + float(guesses[r, 1])]
                    recs = c.all_gather(e.dc_spec(iq_local, base)).cpu().numpy()
                    gathers = 2
                    handoff = {}
                    while True:
                        entries, pending, total = dc_compose(recs, handoff)
                        if pending is None:
                            break
                        ends = c.all_gather(e.dc_resolve(iq_local, entries[pending] if pending == self.rank else None)).cpu().numpy()
                        ends = np.ascontiguousarray(ends).view(np.uint32).reshape(self.world, 2)
                        handoff[pending] = (int(ends[pending, 0]), int(ends[pending, 1]))
                        gathers += 1
                    s = np.array(total, np.uint32).view(np.float32)
                    mean = (s.astype(np.float64) / np.float64(n_total)).astype(np.float32)      # numpy: the float32 sum divided in float64, rounded once
                stats = e.dc_stats()
            res = e.dc_apply(iq_local, mean, out)
        fixed = [e.dc_apply(t, mean, None) for t in also]
        self.last_dc = {"mean": mean, "all_gathers": gathers, **stats}
        return (res, fixed) if also else res

    def iq_to_bits(self, iq_local, p, want_qad=True, pos_base=None, n_total=None, halo_given=False, left_halo=None, left_raw=None, auto_center=False,
                   msg_records=False, dc_correction=False):
        """iq_local: this rank's shard.  pos_base / n_total default to equal shards of len(iq_local).
        halo_given (the same on every rank): whoever distributed the capture handed every rank but the first the two samples that
        precede its shard (left_halo: (2, 2) in the shard's dtype, or complex64 (2,)) -- 16 bytes more per rank to read from the
        file.  The halo exchange is then skipped: two all-gathers per pass (ASK: three) instead of three (four).
        PSK: every rank but the first passes left_raw, the costas_halo_samples(p.costas_loop_bandwidth, pos_base) raw samples
        before its shard ((m, 2) in the shard's dtype, or complex64 (m,); a longer tail is cut to them); halo_given / left_halo do
        not apply.  The pass's Costas exchange is recorded in `last_costas`; the result always carries the shard's qad.
        auto_center (the same on every rank: it adds collectives): a PSK pass calls `detect_center` on the demodulated signal once the
        Costas exchange has written it and builds its pulse table with the detected center (p.center where detection gives None);
        `last_center` is the value used.  ASK / FSK raise ValueError: their fused hot kernel needs the center before the demodulated
        signal exists.  The recipe there is two passes: one with want_qad=True, `detect_center(result.qad)`, then a second pass with
        that center -- or `iq_to_bits_auto(auto_center=True)`, which demodulates the shard once, detects the center across the shards and
        slices from the demodulated signal; it also takes auto_noise (every modulation).
        msg_records: refused (ValueError) as an option of the pass -- a message's middle window may lie in another rank's shard; the recipe is
        iq_to_bits, then `message_records` on the same shard and the pass's result.
        dc_correction: refused (ValueError) as an option of the pass; the recipe is `dc_correct` (the mean of the WHOLE capture, carried
        across the ranks), then iq_to_bits on the result -- with left_halo / left_raw corrected through its `also`."""
        e, c = self.engine, self.comm
        if dc_correction:
            raise ValueError("DC correction is not an option of a sharded pass: call dc_correct on the shard first, then iq_to_bits on the result")
        if msg_records:
            raise ValueError("message records are not an option of a sharded pass: call message_records(iq_local, result, p) after iq_to_bits")
        if auto_center and p.modulation_type != "PSK":
            raise ValueError("auto_center needs a PSK pass: for ASK / FSK run a pass with want_qad=True, detect_center(result.qad), "
                             "then a second pass with that center")
        n_local = int(iq_local.shape[0])
        if pos_base is None:
            pos_base = self.rank * n_local
        if n_total is None:
            n_total = self.world * n_local
        if p.modulation_type == "PSK":
            return self._iq_to_bits_psk(iq_local, p, int(pos_base), int(n_total), left_raw, bool(auto_center))
        self.last_center = p.center
        if halo_given and self.rank > 0 and left_halo is None:
            raise ValueError("halo_given: ranks > 0 pass the two samples before their shard as left_halo")
        pending = left = None
        if not halo_given:
            # the halo exchange overlaps the hot kernel (all chunks but the first); on a pipelined engine it is issued on the tail
            # stream (behind the previous pass's exchanges), which first waits for whatever produced the shard on the caller's stream
            with (e.halo_context() if hasattr(e, "halo_context") else contextlib.nullcontext()):
                pending = c.all_gather_start(e.tail(iq_local, p))
            if hasattr(e, "runs_begin"):
                e.runs_begin(iq_local, pos_base, n_total, self.rank, self.world, p, want_qad)
        else:
            if self.rank > 0:
                left = e.halo_view(left_halo) if hasattr(e, "halo_view") else left_halo
            if hasattr(e, "runs_launch"):          # the whole hot launch, on the hot stream
                e.runs_launch(iq_local, left, pos_base, n_total, self.rank, self.world, p, want_qad)
        # Everything after the hot kernel -- the wait for the halo, the first chunk, the all-gathers -- is issued on the engine's tail
        # stream when it is pipelined: the next pass's hot kernel then overlaps this pass's latency-bound tail, and the hot stream
        # never waits for a collective (the exchanges of one process group run in issue order: the halo of pass i + 1 sits behind the
        # last exchange of pass i's tail, so a hot stream that waited for its halo would run in lock-step with the tails).
        with (e.tail_context() if hasattr(e, "tail_context") else contextlib.nullcontext()):
            if pending is not None:
                halos = pending()
                left = halos[self.rank - 1] if self.rank > 0 else None
            summary = e.runs(iq_local, left, pos_base, n_total, self.rank, self.world, p, want_qad)
            merge = e.rows(c.all_gather(summary))
            merged_all = c.all_gather(merge) if merge is not None else None
            flags = e.bits_prepare(merged_all)
            return e.bits_finish(c.all_gather(flags))

    def iq_to_bits_auto(self, iq_local, p, auto_noise=False, auto_center=False, center_max_size=None, want_qad=True, pos_base=None, n_total=None,
                        halo_given=False, left_halo=None, left_raw=None):
        """The pass of DevicePipeline.iq_to_bits(auto_noise=..., auto_center=..., center_max_size=...) on a sharded capture, bit for bit: the
        same ShardResult as iq_to_bits (stitch, message_records, stitch_records and message_data work on it unchanged).  iq_local, pos_base,
        n_total, halo_given / left_halo, left_raw (PSK), want_qad: as iq_to_bits.
        auto_noise, auto_center and center_max_size MUST BE THE SAME ON EVERY RANK: they add collectives.
        auto_noise: noise = detect_noise_level(iq_local, pos_base, n_total) -- one all-gather, the same value on every rank -- and the pass
        runs with dataclasses.replace(p, noise_threshold=noise).  Where the noise level is not below the sample type's max_magnitude (compared
        as doubles) the reference demodulates nothing (Signal.py:474-484): EVERY rank raises ValueError, decided from the gathered value, and
        none enters a further collective.  What the reference raises for a level that is not a number (math.ceil) is raised on every rank alike.
        auto_center: the pulse table is built with detect_center(demodulated signal of the WHOLE capture, center_max_size); p.center where
        that gives None.  PSK: the PSK pass of iq_to_bits.  ASK / FSK: the shard is demodulated once into the result's qad together with the
        seam value (the demodulated value of the sample before the shard, from the two raw samples of the halo), the center is detected
        across the shards, and runs, rows and bits follow from the qad with that center (module docstring, "Automatic passes").  This route
        needs want_qad=True and an engine that is not pipelined (ValueError otherwise: it reads gathered values on the host).
        Without auto_center, ASK / FSK take the fused pass of iq_to_bits with the replaced parameters (a pipelined engine is fine there).
        Modulations other than ASK, FSK and PSK raise ValueError.  Everything a rank can get wrong on its own is refused before the first
        collective.  `last_center` is the center the pulse table was built with; `last_auto` = {"noise": the detected level or None,
        "center": the center used, "center_detected": whether detect_center found it, "all_gathers": all-gathers of this call}.  ASK / FSK
        with auto_center: the halo's unless halo_given, detect_center's, summaries + (ASK) merge + flags, one more with auto_noise."""
        import dataclasses
        from .sniffer import max_magnitude
        e = self.engine
        auto_noise, auto_center = bool(auto_noise), bool(auto_center)
        mod = p.modulation_type
        if mod not in ("ASK", "FSK", "PSK"):
            raise ValueError(f"iq_to_bits_auto: ASK, FSK and PSK passes only (got {mod})")
        if auto_center and not want_qad:
            raise ValueError("auto_center needs the demodulated signal (want_qad=True)")
        if center_max_size is not None and int(center_max_size) < 0:
            raise ValueError("detect_center: max_size must not be negative")
        n_local = int(iq_local.shape[0])
        pos_base = self.rank * n_local if pos_base is None else int(pos_base)
        n_total = self.world * n_local if n_total is None else int(n_total)
        if pos_base < 0 or pos_base + n_local > n_total:
            raise ValueError("iq_to_bits_auto: the shard does not lie inside the capture")
        psk = mod == "PSK"
        own_route = auto_center and not psk
        # everything this rank can get wrong on its own, now: later refusals would leave the other ranks in a collective
        if auto_noise:
            self._estimator_engine("noise_partials")
        if psk or own_route:
            if n_total <= 2:
                raise ValueError(f"{mod}: a capture of two samples or fewer does not shard")
            if getattr(e, "tail_stream", None) is not None:
                raise ValueError(f"{'PSK shards run' if psk else 'an ASK / FSK pass with auto_center runs'} on an engine that is not pipelined: "
                                 "gathered values are read on the host between the phases")
        if psk:
            if auto_center:
                self._estimator_engine("costas_qad", "set_center", "compact_gt", "pairwise_partial", "histogram")
            if self.rank > 0:
                need = costas_halo_samples(p.costas_loop_bandwidth, pos_base)
                have = 0 if left_raw is None else int(left_raw.shape[0])
                if have < need:
                    raise ValueError(f"PSK: rank {self.rank} needs the {need} raw samples before its shard as left_raw (got {have})")
        else:
            if halo_given and self.rank > 0 and left_halo is None:
                raise ValueError("halo_given: ranks > 0 pass the two samples before their shard as left_halo")
            if own_route:
                self._estimator_engine("demod_own", "demod", "demod_qad", "set_center", "compact_gt", "pairwise_partial", "histogram")
                e.demod_own(iq_local, left_halo if (halo_given and self.rank > 0) else None)
        counted = _CountingComm(self.comm)
        self.comm, comm = counted, self.comm
        try:
            noise = None
            if auto_noise:
                noise = self.detect_noise_level(iq_local, pos_base, n_total)       # raises on every rank alike (gathered statistics)
                dt = str(iq_local.dtype).replace("torch.", "")
                limit = max_magnitude(np.float32 if dt == "complex64" else dt)
                if not (float(noise) < float(limit)):                               # decided from the gathered value: every rank raises
                    raise ValueError(f"iq_to_bits_auto: the detected noise level {float(noise)!r} is not below the sample type's max_magnitude "
                                     f"{float(limit)!r}: the reference demodulates nothing of such a capture (Signal.quad_demod)")
                p = dataclasses.replace(p, noise_threshold=noise)
            self._center_found = False
            if psk:
                res = self._iq_to_bits_psk(iq_local, p, pos_base, n_total, left_raw, auto_center, center_max_size)
            elif not own_route:
                res = self.iq_to_bits(iq_local, p, want_qad=want_qad, pos_base=pos_base, n_total=n_total, halo_given=halo_given, left_halo=left_halo)
            else:
                res = self._iq_to_bits_demod_first(iq_local, p, pos_base, n_total, bool(halo_given), left_halo, center_max_size)
        finally:
            self.comm = comm
        self.last_auto = {"noise": noise, "center": self.last_center, "center_detected": self._center_found, "all_gathers": counted.count}
        return res

    def _iq_to_bits_demod_first(self, iq_local, p, pos_base, n_total, halo_given, left_halo, center_max_size):
        """ASK / FSK with auto_center (module docstring, "Automatic passes"); the caller has checked this rank's arguments"""
        e, c = self.engine, self.comm
        left = None
        if halo_given:
            if self.rank > 0:
                left = e.halo_view(left_halo) if hasattr(e, "halo_view") else left_halo
        else:
            halos = c.all_gather(e.tail(iq_local, p))
            left = halos[self.rank - 1] if self.rank > 0 else None
        e.demod(iq_local, left, pos_base, n_total, self.rank, self.world, p)
        self.last_center = p.center
        center = self.detect_center(e.demod_qad(), center_max_size)
        if center is not None:
            self.last_center = float(center)
            self._center_found = True
            e.set_center(self.last_center)
        summary = e.runs(iq_local, left, pos_base, n_total, self.rank, self.world, p, True)     # from the qad; its left halo is the seam value
        merge = e.rows(c.all_gather(summary))
        flags = e.bits_prepare(c.all_gather(merge) if merge is not None else None)
        return e.bits_finish(c.all_gather(flags))

    def message_records(self, iq_local, result, p, message_length_divisor=1, pos_base=None, n_total=None):
        """One urhgpu_msg_record (protocol.RECORD_DTYPE) per message that closes on this rank, in order, as a numpy structured array: the
        ASK padding to message_length_divisor, the first and the middle bit's position and the RSSI (module docstring, "Message records").
        Called on EVERY rank after iq_to_bits with the shard that pass demodulated (after dc_correct: the corrected shard) and its result;
        pos_base / n_total default as in iq_to_bits.  The ranks' arrays concatenated in rank order are the records of
        DevicePipeline.iq_to_bits(msg_records=True, message_length_divisor=d) on the whole capture, RSSI bit patterns included.  ASK, FSK and
        PSK passes alike; only the padding depends on the modulation.
        Synchronous: gathered words are read on the host.  Two all-gathers, a third where a first message's window is not wholly inside its
        closing rank's shard, none on one rank; shards that do not tile [0, n_total) raise ValueError on every rank (decided from gathered
        data).  A rank that closes no message returns an empty array and takes part in every collective.  `last_records` records the number of
        all-gathers and of exchanged windows.  On a pipelined engine the device work runs behind the pass's tail."""
        e = self._estimator_engine("records_summary", "records_lookup", "records_window_part", "records_finish")
        c = self.comm
        if not p.write_bit_sample_pos:
            raise ValueError("message_records needs the positions of the pass (write_bit_sample_pos)")
        divisor = int(message_length_divisor)
        if divisor < 1 or divisor > 1 << 30:
            raise ValueError("message_records: 1 <= message_length_divisor <= 2^30")
        n_local = int(iq_local.shape[0])
        pos_base = self.rank * n_local if pos_base is None else int(pos_base)
        n_total = self.world * n_local if n_total is None else int(n_total)
        sps = int(p.samples_per_symbol)
        gathers = 0

        def gather(t):
            nonlocal gathers
            if self.world == 1:
                return t[None]
            gathers += 1
            return c.all_gather(t)
        with (e.tail_context() if hasattr(e, "tail_context") else contextlib.nullcontext()):
            words = gather(e.records_summary(iq_local, result, pos_base)).cpu().numpy()
            plan = records_plan(words, n_total, sps, divisor if p.modulation_type == "ASK" else 1)      # raises on every rank alike
            values = gather(e.records_lookup(result, records_requests(plan, self.rank))).cpu().numpy()
            firsts, outside = records_windows(plan, words, values, n_total, sps)
            window = None
            if outside:
                spans = [(firsts[r]["lo"], firsts[r]["w"]) for r in outside]
                parts = gather(e.records_window_part(iq_local, pos_base, spans, max(k for _, k in spans)))
                mine = firsts[self.rank]
                if mine is not None and mine["slot"] >= 0:
                    w = np.ascontiguousarray(np.asarray(words)).view(np.int64).reshape(self.world, REC_SUMMARY_WORDS)
                    lo, hi = mine["lo"], mine["lo"] + mine["w"]
                    window = parts.new_empty((mine["w"],) + tuple(parts.shape[3:]))           # contiguous, in the engine's memory
                    for q in range(self.world):                   # the shards tile the capture: every sample comes from exactly one rank
                        a, b = max(lo, int(w[q, REC_POS_BASE])), min(hi, int(w[q, REC_POS_BASE] + w[q, REC_N_LOCAL]))
                        if b > a:
                            window[a - lo:b - lo] = parts[q, mine["slot"], a - lo:b - lo]
            first = np.zeros(REC_FIRST_WORDS, np.int64)
            m, f = plan[self.rank], firsts[self.rank]
            if m is not None:
                first[:4] = (1, m["L"], m["np"], m["n_pad"])
                if f is not None:
                    first[4:] = (f["first_pos"], f["mid_pos"], 1, 1 if window is not None else 0)
            rec = e.records_finish(iq_local, result, pos_base, n_total, p, divisor, first, window)
        self.last_records = {"all_gathers": gathers, "windows": len(outside)}
        return rec

    def _iq_to_bits_psk(self, iq_local, p, pos_base, n_total, left_raw, auto_center=False, center_max_size=None):
        """the PSK pass (module docstring, steps 0-4).  Everything a rank can get wrong on its own is checked before the first collective."""
        e, c = self.engine, self.comm
        if auto_center:
            self._estimator_engine("costas_qad", "set_center", "compact_gt", "pairwise_partial", "histogram")
        if n_total <= 2:
            raise ValueError("PSK: a capture of two samples or fewer does not shard")
        if self.rank > 0:
            need = costas_halo_samples(p.costas_loop_bandwidth, pos_base)
            have = 0 if left_raw is None else int(left_raw.shape[0])
            if have < need:
                raise ValueError(f"PSK: rank {self.rank} needs the {need} raw samples before its shard as left_raw (got {have})")
            left_raw = left_raw[have - need:]
        else:
            left_raw = None
        summary = e.costas_spec(iq_local, left_raw, pos_base, n_total, self.rank, self.world, p)
        rounds = costas_exchange(c, summary, e.costas_resolve, e.costas_end)
        by_map, by_ckpt, serial, respec = e.costas_stats()
        self.last_costas = {"rounds": rounds, "chunks_by_map": by_map, "chunks_by_checkpoint": by_ckpt, "chunks_serial": serial,
                            "respeculation_rounds": respec}
        lasts = c.all_gather(e.costas_last())                 # every shard's last demodulated value: the seam of the pulse table
        left = lasts[self.rank - 1] if self.rank > 0 else None
        self.last_center = p.center
        if auto_center:
            center = self.detect_center(e.costas_qad(), center_max_size)
            if center is not None:
                self.last_center = float(center)
                self._center_found = True
                e.set_center(self.last_center)
        summary = e.runs(iq_local, left, pos_base, n_total, self.rank, self.world, p, True)
        merge = e.rows(c.all_gather(summary))
        flags = e.bits_prepare(c.all_gather(merge) if merge is not None else None)
        return e.bits_finish(c.all_gather(flags))


def stitch(pieces):
    """Concatenate the per-rank pieces (rank order) of a sharded result into the single-GPU / reference
    shaped flat result.  pieces[r] = dict(rows, bits, msg_end, pauses, pos, pos_end) of numpy arrays, where
    msg_end / pos_end are LOCAL end offsets (in that rank's bits / pos) of the messages that close on rank r.
    Returns (ppseq, bits, msg_off, pauses, pos, pos_off)."""
    rows = np.concatenate([np.asarray(p["rows"], dtype=np.int64).reshape(-1, 2) for p in pieces])
    bits = np.concatenate([np.asarray(p["bits"], dtype=np.uint8) for p in pieces])
    pos = np.concatenate([np.asarray(p["pos"], dtype=np.int64) for p in pieces])
    pauses = np.concatenate([np.asarray(p["pauses"], dtype=np.int64) for p in pieces])
    msg_off, pos_off = [0], [0]
    b0 = p0 = 0
    for p in pieces:
        msg_off.extend((b0 + np.asarray(p["msg_end"], dtype=np.int64)).tolist())
        pos_off.extend((p0 + np.asarray(p["pos_end"], dtype=np.int64)).tolist())
        b0 += len(p["bits"])
        p0 += len(p["pos"])
    return rows, bits, np.array(msg_off, np.int64), pauses, pos, np.array(pos_off, np.int64)


def stitch_records(records):
    """the ranks' record arrays (rank order) as the one array of the whole capture's messages"""
    from .protocol import RECORD_DTYPE
    parts = [np.asarray(r, dtype=RECORD_DTYPE) for r in records]
    return np.concatenate(parts) if parts else np.zeros(0, RECORD_DTYPE)


def message_data(pieces, records, p, sample_rate=1e6, timestamp=0.0):
    """The list of protocol.MessageData of a sharded pass -- what BitsResult.message_data() gives for the single-GPU one -- from the ranks'
    pieces (as `stitch` takes them) and their records (the ranks' arrays in rank order, or one stitched array).  Raises as the single-GPU
    route does (UrhGpuError, ERR_CAPACITY) where a record says that a capacity was exceeded (flag 0), and RuntimeError naming the flag for
    -2 (a window left its rank's shard) and -1."""
    from . import _lib
    from .protocol import messages_from_records
    rec = stitch_records(records) if isinstance(records, (list, tuple)) else np.asarray(records)
    flat = stitch(pieces)[1:]
    if len(rec) != len(flat[2]):
        raise ValueError(f"message_data: {len(rec)} records for {len(flat[2])} messages")
    if not (rec["flag"] == 1).all():
        bad = np.nonzero(rec["flag"] != 1)[0]
        flag = int(rec["flag"][bad[0]])
        where = f"{len(bad)} of {len(rec)} records are not valid (first: message {int(bad[0])}, flag {flag}, record {rec[bad[0]]})"
        if flag == 0:
            raise _lib.UrhGpuError(_lib.ERR_CAPACITY, f"output capacity too small on a rank that contributes to the message: {where}")
        if flag == -2:
            raise RuntimeError(f"message_records: the middle window of a message that is not the first one its rank closes left the rank's shard "
                               f"(flag -2; nothing outside the shard was read, no RSSI): {where}")
        raise RuntimeError(f"message_records: the summation of a window gave up (flag -1): {where}")
    return messages_from_records(flat, rec, p, sample_rate, timestamp)
