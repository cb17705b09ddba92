"""ctypes binding of include/hsrans_hip.h.

Mirrors the reference's codec interface (src/main.cpp:146-155): ``encode(bytes) -> stream`` and
``decode(stream) -> bytes`` selected by container (raw / block_ / mt_), state count (32 / 64) and histogram bits
(10..15) — the three things the reference encodes in its function names
(``rANS32x64_16w_decode_scalar_11``, ``mt_rANS32x32_16w_decode_14`` …).  Failure (the reference's ``return 0``) raises
``HsransError``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch  # first: pins the HIP runtime (libamdhip64.so.7) this process uses before our library is loaded

from ._abi import (  # noqa: F401  (the structures, constants and loader are spelled api.<name> by the tests and tools)
    BLOCK, COMM_ID_BYTES, ENC_INDEPENDENT_BLOCKS, MT, PACK_CHUNK, PACK_MAX_ITEMS, PLANES_MAX, PLANES_STORE_INCOMPRESSIBLE, RAW, SHARD_DECODE_AND_EXCHANGE, SHARD_DECODE_ONLY,
    SHARD_EXCHANGE_ONLY, BatchInfo, Calibration, EncodeBatchStats, EncodeExBatchStats, EncodeExMember, EncodeMember, EncodeOpts, GatherBatchTask,
    GatherMember, GatherSetInfo, GatherTask, Hist, HsransError, IndexingBatchStats, IndexingMember, LaunchFacts, LaunchInfo, MemberRange, PlanKind,
    PlanesBatchStats, PlanesDesc, PlanesGatherBatchTask, PlanesGatherIndirectInfo, PlanesGatherInfo, PlanesGatherSetIndirectInfo, PlanesGatherSetInfo, PlanesGatherTask, PlanesInfo, PlanesMember,
    PlanesSetInfo, QueueStats, Range, Shard, ShardedInfo, _sz, _vp, lib_path, load_library)


def _u8(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8) if not isinstance(a, (bytes, bytearray, memoryview)) else np.frombuffer(a, dtype=np.uint8)
    return a


def _p(a: np.ndarray):
    return a.ctypes.data_as(_vp)


def _check(rc: int, what: str, suffix: str = ""):
    """a C return code that is not HSRANS_OK raises HsransError("<what> failed with code <rc><suffix>") carrying it as ``.code``"""
    if rc != 0:
        raise HsransError(f"{what} failed with code {rc}{suffix}", code=rc)


def _members_error(what: str, rc: int, failed, **got) -> HsransError:
    """the error of a call over many members: names the first of ``failed`` (empty: none to name) and carries what the members got"""
    err = HsransError(f"{what} failed with code {rc}" + (f": member {failed[0]} failed" if failed else ""), code=rc)
    vars(err).update(got)
    return err


def _encode_member(entry: str, k: int, m, known) -> tuple:
    """member k of a batch encoder as (container, states, bits, d_in, d_out, options dict); an option that is not ``known`` raises"""
    o = dict(m[5]) if len(m) > 5 and m[5] is not None else {}
    unknown = set(o) - set(known)
    if unknown:
        raise HsransError(f"{entry}: member {k}: unknown options {sorted(unknown)}")
    return (*m[:5], o)


def _torch_stream(stream, device=None):
    return stream if stream is not None else torch.cuda.current_stream(device)


def _stream(stream, device=None):
    """the hipStream_t a C call takes: ``stream``, or torch's current stream on ``device`` (None: on the current device)"""
    return _vp(_torch_stream(stream, device).cuda_stream)


def _as_dict(s: ctypes.Structure) -> dict:
    """the fields of a structure in their order: arrays as lists, scalars as they are"""
    values = ((n, getattr(s, n)) for n, _ in s._fields_)
    return {n: (list(v) if isinstance(v, ctypes.Array) else v) for n, v in values}


def _handle_array(plans, size: int | None = None):
    """the C array of the plans' handles (NULL for None), of ``size`` entries where that is more than the plans"""
    handles = [None if d is None else (d.handle.value if isinstance(d.handle, _vp) else d.handle) for d in plans]
    return (_vp * (len(handles) if size is None else size))(*handles)


def _tensor_arrays(tensors, lengths=None):
    """(data pointers, lengths) of a list of tensors as C arrays; a tensor's length is lengths[k] where given, else its numel()"""
    K = len(tensors)
    return (_vp * K)(*[t.data_ptr() for t in tensors]), (_sz * K)(*[(t.numel() if lengths is None else int(lengths[k])) for k, t in enumerate(tensors)])


def _indirect_args(d_ranges, columns: int, count, max_count, workspace, workspace_bytes, device, stream):
    """What the *_indirect calls check of their device-side ranges, and their workspace: returns (max_count, workspace) with max_count
    defaulting to the rows of ``d_ranges`` and the workspace, where None, allocated on ``device`` under ``stream`` (``workspace_bytes``:
    max_count -> bytes)."""
    if not (d_ranges.is_cuda and d_ranges.dim() == 2 and d_ranges.shape[1] == columns and d_ranges.dtype in (torch.int64, torch.uint64) and d_ranges.is_contiguous()):
        raise TypeError(f"d_ranges: a contiguous CUDA tensor (N, {columns}) of int64 or uint64")
    if count is not None and not (count.is_cuda and count.numel() == 1 and count.dtype in (torch.int32, torch.uint32)):
        raise TypeError("count: a CUDA int32 or uint32 scalar tensor")
    if max_count is None:
        max_count = d_ranges.shape[0]
    if max_count > d_ranges.shape[0]:
        raise ValueError("max_count is larger than d_ranges")
    if workspace is None:
        with torch.cuda.stream(_torch_stream(stream, device)):
            workspace = torch.empty(workspace_bytes(max_count), dtype=torch.uint8, device=device)
    if not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise TypeError("workspace: a contiguous CUDA uint8 tensor")
    return max_count, workspace


# ---------------------------------------------------------------------------------------------------------------------
# host-side format functions
# ---------------------------------------------------------------------------------------------------------------------
def capacity(container: int, states: int, n: int) -> int:
    return load_library().hsrans_capacity(container, states, n)


def make_hist(data, bits: int) -> Hist:
    data = _u8(data)
    h = Hist()
    load_library().hsrans_make_hist(ctypes.byref(h), _p(data), data.size, bits)
    return h


def hist_from_counts(counts) -> Hist:
    h = Hist()
    run = 0
    for k in range(256):
        h.symbolCount[k] = int(counts[k])
        h.cumul[k] = run & 0xFFFF
        run += int(counts[k])
    return h


def index_boundaries(states: int, bits: int, decoded_size: int, ctx: "Context | None" = None) -> np.ndarray:
    """Checkpoint positions (group indices) for ONE chain per resident wavefront (hsrans_index_boundaries); ctx None = MI355X defaults."""
    out = np.zeros(1 << 16, np.uint64)
    n = load_library().hsrans_index_boundaries(ctx.handle if ctx is not None else None, states, bits, decoded_size, _p(out), out.size)
    return out[:n].copy()


def encode(container: int, states: int, bits: int, data, hist: Hist | None = None, block_size: int = 0, index_interval: int = 0,
           independent_blocks: bool = False, index_groups=None, out_capacity: int | None = None):
    """Returns ``stream`` (np.uint8) or ``(stream, plan)`` when ``index_interval`` != 0 or ``index_groups`` (explicit checkpoints) is given.
    ``out_capacity``: room for the stream when a caller-made histogram makes the data EXPAND (default: the reference's capacity)."""
    L = load_library()
    data = _u8(data)
    cap = L.hsrans_capacity(container, states, data.size) if out_capacity is None else int(out_capacity)
    out = np.zeros(cap, np.uint8)
    hp = ctypes.byref(hist) if hist is not None else None
    if index_groups is not None:
        index_groups = np.ascontiguousarray(index_groups, dtype=np.uint64)
        if index_groups.size == 0:  # a stream too short for more than one chain
            index_groups, index_interval = None, 4
    want_plan = index_interval != 0 or index_groups is not None
    if not want_plan and block_size == 0 and not independent_blocks:
        m = L.hsrans_encode(container, states, bits, _p(data), data.size, _p(out), cap, hp)
        if m == 0:
            raise HsransError("encode failed")
        return out[:m].copy()
    if index_groups is not None:
        pcap = L.hsrans_plan_capacity_chains(container, states, data.size, index_groups.size, block_size)
    else:
        pcap = L.hsrans_plan_capacity(container, states, data.size, index_interval, block_size) if index_interval else 0
    plan = np.zeros(max(pcap, 1), np.uint8)
    opts = EncodeOpts(block_size, 0 if index_groups is not None else index_interval, plan.ctypes.data if want_plan else None, pcap, 0,
                      ENC_INDEPENDENT_BLOCKS if independent_blocks else 0, 0, index_groups.ctypes.data if index_groups is not None else None,
                      index_groups.size if index_groups is not None else 0)
    m = L.hsrans_encode_ex(container, states, bits, _p(data), data.size, _p(out), cap, hp, ctypes.byref(opts))
    if m == 0:
        raise HsransError("encode failed")
    if not want_plan:
        return out[:m].copy()
    return out[:m].copy(), plan[:opts.plan_size].copy()


BLOCK_CHOICE = np.dtype([("begin", np.uint64), ("end", np.uint64), ("single", np.uint32), ("symbol", np.uint32), ("counts", np.uint16, 256)])


def block_choices(container: int, states: int, bits: int, data, block_size: int = 0) -> np.ndarray:
    """The host encoder's block choice for block_/mt_ (hsrans_block_choices): a BLOCK_CHOICE record per block, in stream order."""
    L = load_library()
    data = _u8(data)
    n = L.hsrans_block_choices(container, states, bits, _p(data), data.size, block_size, None, 0)
    if n == 0:
        raise HsransError("hsrans_block_choices failed")
    out = np.zeros(n, BLOCK_CHOICE)
    L.hsrans_block_choices(container, states, bits, _p(data), data.size, block_size, out.ctypes.data, n)
    return out


def plan_thin(plan, groups) -> np.ndarray:
    plan = _u8(plan)
    groups = np.ascontiguousarray(groups, dtype=np.uint64)
    out = np.zeros(plan.size, np.uint8)
    n = load_library().hsrans_plan_thin(_p(plan), plan.size, _p(groups), groups.size, _p(out), out.size)
    if n == 0:
        raise HsransError("plan_thin failed")
    return out[:n].copy()


def plan_build(container: int, states: int, bits: int, stream, out_capacity: int | None = None) -> np.ndarray:
    L = load_library()
    stream = _u8(stream)
    if stream.size < 16:
        raise HsransError("stream too short")
    out_len = int(stream[:8].view(np.uint64)[0])
    if out_capacity is None:
        out_capacity = out_len
    pcap = L.hsrans_plan_capacity(container, states, min(out_len, 1 << 40), 0, 0)
    plan = np.zeros(pcap, np.uint8)
    n = L.hsrans_plan_build(container, states, bits, _p(stream), stream.size, out_capacity, _p(plan), pcap)
    if n == 0 and container != RAW:
        # blocks below the 32 KiB hsrans_plan_capacity assumes for foreign streams (encode(block_size=...)): one chain per
        # block header of the stream at most
        pcap = min(L.hsrans_plan_capacity(container, states, min(out_len, 1 << 40), 0, 64), stream.size * 40 + (1 << 20))
        plan = np.zeros(pcap, np.uint8)
        n = L.hsrans_plan_build(container, states, bits, _p(stream), stream.size, out_capacity, _p(plan), pcap)
    if n == 0:
        raise HsransError("malformed stream (plan_build returned 0)")
    return plan[:n].copy()


def plan_chain_count(plan) -> int:
    plan = _u8(plan)
    return load_library().hsrans_plan_chain_count(_p(plan), plan.size)


def plan_decoded_length(plan) -> int:
    plan = _u8(plan)
    return load_library().hsrans_plan_decoded_length(_p(plan), plan.size)


def plan_slice(plan, first: int, count: int) -> np.ndarray:
    plan = _u8(plan)
    out = np.zeros(plan.size, np.uint8)
    n = load_library().hsrans_plan_slice(_p(plan), plan.size, first, count, _p(out), out.size)
    if n == 0:
        raise HsransError("plan_slice failed")
    return out[:n].copy()


def plan_chain_range(plan, first: int, count: int) -> tuple[int, int]:
    plan = _u8(plan)
    b, e = ctypes.c_uint64(), ctypes.c_uint64()
    rc = load_library().hsrans_plan_chain_range(_p(plan), plan.size, first, count, ctypes.byref(b), ctypes.byref(e))
    if rc != 0:
        raise HsransError("plan_chain_range failed", code=rc)
    return b.value, e.value


def plan_stream_ranges(plan, first: int, count: int) -> tuple[tuple[int, int], tuple[int, int]]:
    """((head_begin, head_end), (body_begin, body_end)): the stream bytes chains [first, first+count) can read."""
    plan = _u8(plan)
    r = (ctypes.c_uint64 * 4)()
    rc = load_library().hsrans_plan_stream_ranges(_p(plan), plan.size, first, count, r)
    if rc != 0:
        raise HsransError("plan_stream_ranges failed", code=rc)
    return (r[0], r[1]), (r[2], r[3])


# ---------------------------------------------------------------------------------------------------------------------
# host SIMD decoders (csrc/hsrans_cpu.cpp): the CPU comparator / single-chain path; never used by Context (the GPU entries)
# ---------------------------------------------------------------------------------------------------------------------
CPU_LEVELS = {0: "scalar", 1: "avx2", 2: "avx512"}


def cpu_level() -> int:
    return load_library().hsrans_cpu_level()


def decode_cpu(container: int, states: int, bits: int, stream, out_capacity: int | None = None, plan=None, level: int = -1, threads: int = 1,
               in_length: int | None = None):
    """Returns (returned_length, out) like the reference's decoders (0 = failure).  hsrans_decode_cpu."""
    stream = _u8(stream)
    if out_capacity is None:
        out_capacity = int(stream[:8].view(np.uint64)[0]) if stream.size >= 8 else 0
    out = np.full(max(out_capacity, 1) + 64, 0xCC, np.uint8)
    pp, pn = (None, 0)
    if plan is not None:
        plan = _u8(plan)
        pp, pn = _p(plan), plan.size
    r = load_library().hsrans_decode_cpu(level, threads, container, states, bits, _p(stream), stream.size if in_length is None else in_length, _p(out),
                                         out_capacity, pp, pn)
    return r, out[:out_capacity]


def index_build_host(container: int, states: int, bits: int, stream, groups, level: int = -1, threads: int = 1) -> np.ndarray:
    stream = _u8(stream)
    groups = np.ascontiguousarray(groups, dtype=np.uint64)
    out_len = int(stream[:8].view(np.uint64)[0])
    L = load_library()
    pcap = L.hsrans_plan_capacity_chains(container, states, out_len, groups.size, 0)
    plan = np.zeros(pcap, np.uint8)
    n = L.hsrans_index_build_host(level, threads, container, states, bits, _p(stream), stream.size, _p(groups), groups.size, _p(plan), pcap)
    if n == 0:
        raise HsransError("hsrans_index_build_host failed")
    return plan[:n].copy()


PIECE_DTYPE = np.dtype([("words_off", "<u8"), ("out_off", "<u8"), ("hist_off", "<u8"), ("fill_len", "<u8"), ("steps", "<u4"),
                        ("tail", "<u2"), ("flags", "<u2"), ("state_idx", "<u4"), ("reserved", "<u4")])


def plan_tables(plan):
    """Read-only numpy views of a plan blob (layout: csrc/hsrans_plan.h): (header dict, chain_first[n+1], pieces[n_pieces])."""
    plan = _u8(plan)
    if plan.size < 64 or bytes(plan[:8]) != b"HSRPLAN1":
        raise HsransError("not a plan blob")
    u32 = plan[8:24].view("<u4")
    hdr = {"container": int(u32[0]), "states": int(u32[1]), "bits": int(u32[2]), "flags": int(u32[3]),
           "decoded_len": int(plan[24:32].view("<u8")[0]), "stream_len": int(plan[32:40].view("<u8")[0]),
           "n_chains": int(plan[40:44].view("<u4")[0]), "n_pieces": int(plan[44:48].view("<u4")[0]),
           "shared_hist": int(plan[48:52].view("<u4")[0]), "interval": int(plan[52:56].view("<u4")[0])}
    nc, npc = hdr["n_chains"], hdr["n_pieces"]
    cf = plan[64:64 + 4 * (nc + 1)].view("<u4")
    po = 64 + ((nc + 1) * 4 + 15) // 16 * 16
    pieces = plan[po:po + 48 * npc].view(PIECE_DTYPE)
    return hdr, cf, pieces


def dealt_shares(block_begin, total_groups: int, ctx: "Context | None" = None, bits: int = 11):
    """hsrans_dealt_shares: (suits the launch?, begin[513], split[512]) for a plan whose block k is chains [block_begin[k], block_begin[k + 1])"""
    bb = np.ascontiguousarray(block_begin, dtype=np.uint32)
    begin, split = np.zeros(513, np.uint32), np.zeros(512, np.uint16)
    rc = load_library().hsrans_dealt_shares(ctx.handle if ctx is not None else None, bits, _p(bb), bb.size - 1, int(bb[-1]), int(total_groups), _p(begin), _p(split))
    if rc < 0:
        raise HsransError("hsrans_dealt_shares: bad arguments", code=rc)
    return rc == 1, begin, split


def launch_choice(plan: dict, ctx: "Context | None" = None, **facts):
    """hsrans_launch_choice: (kernel name, launch_info dict) of the single-plan decode launch a plan of these header fields (``plan``: PlanKind's
    fields, 0 where left out) and launch facts (LaunchFacts' fields as keywords) would get; raises NotImplementedError / ValueError where the
    launcher refuses it as not supported / as an invalid value."""
    info, name = LaunchInfo(), ctypes.create_string_buffer(128)
    rc = load_library().hsrans_launch_choice(ctx.handle if ctx is not None else None, ctypes.byref(PlanKind(**plan)), ctypes.byref(LaunchFacts(**facts)), ctypes.byref(info),
                                             name, len(name))
    if rc == 1:
        raise NotImplementedError("hsrans_launch_choice: no kernel takes this launch")
    if rc == 2:
        raise ValueError("hsrans_launch_choice: the launcher refuses these values")
    if rc != 0:
        raise HsransError("hsrans_launch_choice: bad arguments", code=rc)
    return name.value.decode(), _as_dict(info)


def index_boundaries_batch(states: int, bits: int, decoded_sizes, member: int, ctx: "Context | None" = None) -> np.ndarray:
    """hsrans_index_boundaries_batch: checkpoint positions for member ``member`` of a batch of streams of ``decoded_sizes``."""
    sizes = (ctypes.c_size_t * len(decoded_sizes))(*[int(x) for x in decoded_sizes])
    out = np.zeros(1 << 15, np.uint64)
    n = load_library().hsrans_index_boundaries_batch(ctx.handle if ctx is not None else None, states, bits, sizes, len(decoded_sizes), member, _p(out), out.size)
    return out[:n].copy()


def shard_layout(plan, world: int, parts: int = 1, weights=None):
    """hsrans_shard_layout: (shards[world][parts] as (first_chain, chain_count, out_begin, out_end), windows[world] as (begin, end)).
    Pure host arithmetic in the C library — what every rank of a sharded decode computes identically."""
    plan = _u8(plan)
    shards = (Shard * (world * parts))()
    windows = np.zeros(2 * world, np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.size != world:
        raise HsransError("shard_layout: one weight per rank")
    _check(load_library().hsrans_shard_layout(_p(plan), plan.size, world, parts, None if w is None else _p(w), shards, _p(windows)), "hsrans_shard_layout")
    out = [[(int(shards[r * parts + k].first_chain), int(shards[r * parts + k].chain_count), int(shards[r * parts + k].out_begin), int(shards[r * parts + k].out_end))
            for k in range(parts)] for r in range(world)]
    return out, [(int(windows[2 * r]), int(windows[2 * r + 1])) for r in range(world)]


def _ranges_array(ranges) -> np.ndarray:
    """(N, 3) uint64, C-contiguous: the memory layout of hsrans_range[N]"""
    arr = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 3))
    return arr


def gather_segment(decoded_len: int, n_chains: int, states: int, interval: int) -> int:
    """hsrans_gather_segment: the segment length L a gather's ranges are cut at (absolute multiples of it); 0 for n_chains == 0."""
    return int(load_library().hsrans_gather_segment(decoded_len, n_chains, states, interval))


def gather_workspace_bytes(max_count: int) -> int:
    """hsrans_gather_workspace_bytes: the device workspace a decode_device_gather_indirect of up to ``max_count`` ranges needs."""
    return int(load_library().hsrans_gather_workspace_bytes(max_count))


def gather_batch_workspace_bytes(members: int, max_count: int) -> int:
    """hsrans_gather_batch_workspace_bytes: the device workspace a decode_device_gather_batch_indirect of up to ``max_count`` ranges on a
    gather set of ``members`` members needs; 0 for members == 0 or above 65,536."""
    return int(load_library().hsrans_gather_batch_workspace_bytes(members, max_count))


def gather_tasks(decoded_len: int, n_chains: int, states: int, interval: int, ranges, capacity: int | None = None) -> np.ndarray:
    """hsrans_gather_tasks: the one-wave tasks ``ranges`` ((N, 3) uint64 or a list of (offset, length, dst_offset)) are cut into, as an
    (M, 3) array of (begin, end, dst_delta) (dst_delta as uint64, modulo 2^64).  Pure host arithmetic; an empty array for invalid input.
    ``capacity``: write at most so many tasks (the C call's protocol: the array then holds min(capacity, M) rows)."""
    L = load_library()
    arr = _ranges_array(ranges)
    n = L.hsrans_gather_tasks(decoded_len, n_chains, states, interval, _p(arr) if arr.size else None, arr.shape[0], None, 0)
    rows = n if capacity is None else min(n, capacity)
    out = np.zeros((rows, 3), np.uint64)
    if rows:
        L.hsrans_gather_tasks(decoded_len, n_chains, states, interval, _p(arr), arr.shape[0], _p(out), rows)
    return out


def _member_ranges_array(ranges) -> np.ndarray:
    """rows (member, offset, length, dst_offset) -> hsrans_member_range[N] as a structured array (reserved = 0)"""
    rows = np.asarray(ranges, dtype=np.uint64).reshape(-1, 4)
    if rows.size and int(rows[:, 0].max()) > 0xFFFFFFFF:
        raise ValueError("member does not fit 32 bits")
    arr = np.zeros(rows.shape[0], np.dtype([("offset", "<u8"), ("length", "<u8"), ("dst_offset", "<u8"), ("member", "<u4"), ("reserved", "<u4")]))
    arr["member"], arr["offset"], arr["length"], arr["dst_offset"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    return arr


def gather_batch_tasks(members, ranges, kind: int, waves: int, capacity: int | None = None) -> np.ndarray:
    """hsrans_gather_batch_tasks: the entries of the launch of one ``kind`` (0..5; 3..5: one table per workgroup, the entries sorted by member
    and every member's run padded to a multiple of ``waves``) for ``members`` (rows (decoded_len, n_chains, states, interval, kind)) and
    ``ranges`` (rows (member, offset, length, dst_offset)), as an (M, 4) uint64 array of (begin, end, dst_delta modulo 2^64, member).  Pure
    host arithmetic; an empty array for invalid input.  ``capacity``: as gather_tasks."""
    L = load_library()
    rows = np.asarray(members, dtype=np.uint64).reshape(-1, 5)
    mem = np.zeros(rows.shape[0], np.dtype([("decoded_len", "<u8"), ("n_chains", "<u4"), ("states", "<u4"), ("interval", "<u4"), ("kind", "<u4")]))
    for k, name in enumerate(mem.dtype.names):
        mem[name] = rows[:, k]
    arr = _member_ranges_array(ranges)
    n = L.hsrans_gather_batch_tasks(_p(mem) if mem.size else None, mem.shape[0], _p(arr) if arr.size else None, arr.shape[0], kind, waves, None, 0)
    rows_out = n if capacity is None else min(n, capacity)
    out = np.zeros(rows_out, np.dtype([("begin", "<u8"), ("end", "<u8"), ("dst_delta", "<u8"), ("member", "<u4"), ("reserved", "<u4")]))
    if rows_out:
        L.hsrans_gather_batch_tasks(_p(mem), mem.shape[0], _p(arr), arr.shape[0], kind, waves, _p(out), rows_out)
    return np.stack([out["begin"], out["end"], out["dst_delta"], out["member"].astype(np.uint64)], axis=1) if rows_out else np.zeros((0, 4), np.uint64)


def batch_deal(chain_starts, grid: int = 512, waves: int = 16, weights=None):
    """hsrans_batch_deal: how one launch's wave slots would be dealt to members whose chains start at ``chain_starts[m]`` (groups,
    ascending, last entry = the member's total).  Returns (imbalance, slots[grid * waves, 4] = member, first chain, end chain, flags)."""
    L = load_library()
    arrs = [np.ascontiguousarray(c, dtype=np.uint64) for c in chain_starts]
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    n_chains = np.array([a.size - 1 for a in arrs], np.uint32)
    slots = np.zeros(grid * waves * 4, np.uint32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    imb = L.hsrans_batch_deal(ptrs, _p(n_chains), len(arrs), grid, waves, None if w is None else _p(w), _p(slots))
    if imb < 0:
        raise HsransError("hsrans_batch_deal: bad arguments")
    return float(imb), slots.reshape(-1, 4)


def planes_capacity(itemsize: int, states: int, elements: int) -> int:
    """hsrans_planes_capacity: the bytes of a frame of ``elements`` elements of ``itemsize`` bytes (0: bad arguments)."""
    return load_library().hsrans_planes_capacity(itemsize, states, elements)


def planes_workspace_bytes(itemsize: int, elements: int) -> int:
    """hsrans_planes_workspace_bytes: the workspace of encode_device_planes / decode_device_planes (0: bad arguments)."""
    return load_library().hsrans_planes_workspace_bytes(itemsize, elements)


def planes_batch_workspace_bytes(itemsizes, elements) -> int:
    """hsrans_planes_batch_workspace_bytes: the workspace of encode_device_planes_batch / decode_device_planes_batch over tensors of
    ``itemsizes[k]``-byte items and ``elements[k]`` elements — the sum of the members' planes_workspace_bytes (0: a bad member, no member,
    lists of different lengths, an overflow)."""
    itemsizes, elements = list(itemsizes), list(elements)
    if len(itemsizes) != len(elements) or any(not 0 <= int(v) < 1 << 32 for v in itemsizes) or any(not 0 <= int(v) < 1 << 64 for v in elements):
        return 0
    K = len(elements)
    return int(load_library().hsrans_planes_batch_workspace_bytes((ctypes.c_uint32 * max(K, 1))(*itemsizes), (_sz * max(K, 1))(*elements), K))


def planes_batch_tasks(elements) -> tuple:
    """hsrans_planes_batch_tasks: ``(total, first_task)`` — the workgroups of the one split or merge launch over tensors of ``elements[k]``
    elements and their exclusive prefix (K + 1 entries, the last the total).  ``(0, [])``: no member, a member without elements or with
    more than 2^42, or 2^31 tasks or more."""
    elements = list(elements)
    K = len(elements)
    if any(not 0 <= int(v) < 1 << 64 for v in elements):
        return 0, []
    first = (ctypes.c_uint32 * (K + 1))()
    total = int(load_library().hsrans_planes_batch_tasks((_sz * max(K, 1))(*elements), K, first))
    return total, (list(first) if total else [])


def _pack_lengths(lengths):
    """the C array of an arena's item lengths, None where no call could take them (too many, or a value no size_t holds)"""
    lengths = list(lengths)
    if len(lengths) > PACK_MAX_ITEMS or any(not 0 <= int(v) < 1 << 64 for v in lengths):
        return None, 0
    return (_sz * max(len(lengths), 1))(*[int(v) for v in lengths]), len(lengths)


def _pack_buffers(entry: str, tensors):
    """what the pack wrappers ask of their sources and their arena: CUDA uint8 tensors, contiguous, so that numel() is their bytes"""
    if any(not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()) for t in tensors):
        raise TypeError(f"{entry}: the sources and the arena are contiguous CUDA uint8 tensors")


def pack_layout(lengths) -> tuple:
    """hsrans_pack_layout: ``(total, offsets)`` — the exact bytes of an arena that holds items of ``lengths[k]`` bytes, each at a multiple
    of 16, and where they begin (K + 1 entries, the last the total).  ``(0, [])``: no item, an item of 0 bytes, more than 524,288 items,
    or an overflow."""
    arr, K = _pack_lengths(lengths)
    if arr is None:
        return 0, []
    offsets = (ctypes.c_uint64 * (K + 1))()
    total = int(load_library().hsrans_pack_layout(arr, K, offsets))
    return total, (list(offsets) if total else [])


def pack_tasks(lengths) -> tuple:
    """hsrans_pack_tasks: ``(total, first_task)`` — the workgroups of the one pack launch over items of ``lengths[k]`` bytes
    (ceil(up16(length) / PACK_CHUNK) each) and their exclusive prefix.  ``(0, [])``: what pack_layout refuses, or 2^31 tasks or more."""
    arr, K = _pack_lengths(lengths)
    if arr is None:
        return 0, []
    first = (ctypes.c_uint32 * (K + 1))()
    total = int(load_library().hsrans_pack_tasks(arr, K, first))
    return total, (list(first) if total else [])


def planes_pack_layout(descs) -> tuple:
    """hsrans_planes_pack_layout: ``(descs, bases, total)`` — the descriptors of the frames packed plane after plane (offsets
    member-relative, every plane at a multiple of 16), where each member's frame begins in the arena (K + 1 entries, the last the total)
    and the arena's exact bytes.  ``([], [], 0)``: no member, more than 65,536, a descriptor hsrans_planes_create's rules refuse, an overflow."""
    descs = list(descs)
    K = len(descs)
    if K == 0 or K > 65536:
        return [], [], 0
    src, out = (PlanesDesc * K)(*descs), (PlanesDesc * K)()
    bases = (ctypes.c_uint64 * (K + 1))()
    total = int(load_library().hsrans_planes_pack_layout(src, K, out, bases))
    return ([PlanesDesc.from_buffer_copy(d) for d in out], list(bases), total) if total else ([], [], 0)


def planes_split(array) -> list:
    """hsrans_planes_split on the host: the byte planes of a contiguous array of 2-, 4- or 8-byte items (plane p = byte p of every
    item, in memory order), a uint8 array of ``array.size`` bytes each."""
    a = np.ascontiguousarray(array)
    planes = [np.empty(a.size, np.uint8) for _ in range(a.itemsize)]
    ptrs = (_vp * max(len(planes), 1))(*[p.ctypes.data for p in planes])
    _check(load_library().hsrans_planes_split(a.itemsize, a.ctypes.data if a.size else ptrs, a.size, ptrs), "hsrans_planes_split")
    return planes


def planes_merge(planes, itemsize: int) -> np.ndarray:
    """hsrans_planes_merge on the host: ``itemsize`` planes of equal length interleaved back into the items' bytes (uint8)."""
    planes = [_u8(p) for p in planes]
    if len(planes) != itemsize or any(p.size != planes[0].size for p in planes):
        raise HsransError("planes_merge: one plane per byte of an item, all of one length")
    out = np.empty(planes[0].size * itemsize, np.uint8)
    ptrs = (_vp * itemsize)(*[p.ctypes.data for p in planes])
    _check(load_library().hsrans_planes_merge(itemsize, ptrs, planes[0].size, out.ctypes.data if out.size else ptrs), "hsrans_planes_merge")
    return out


def planes_split_delta(array, base) -> list:
    """hsrans_planes_split_delta on the host: the byte planes of ``array ^ base`` (two contiguous arrays of the same item size and
    count, XORed byte by byte), as ``planes_split`` gives them."""
    return _planes_split_against("planes_split_delta", array, base)


def planes_merge_delta(planes, base) -> np.ndarray:
    """hsrans_planes_merge_delta on the host: the planes interleaved back into items' bytes and XORed with ``base``'s (a contiguous
    array of ``len(planes)``-byte items, as many as a plane has bytes): uint8."""
    return _planes_merge_against("planes_merge_delta", planes, base)


def planes_split_diff(array, base) -> list:
    """hsrans_planes_split_diff on the host: the byte planes of z, the zigzag of ``array - base`` (two contiguous arrays of the same
    item size and count, their items read as little-endian unsigned integers, the difference modulo 2^(8 * itemsize) with its sign
    folded into the lowest bit), as ``planes_split`` gives them."""
    return _planes_split_against("planes_split_diff", array, base)


def planes_merge_diff(planes, base) -> np.ndarray:
    """hsrans_planes_merge_diff on the host: the planes interleaved back into z, the zigzag undone and the difference added to
    ``base``'s items (a contiguous array of ``len(planes)``-byte items, as many as a plane has bytes): the items' bytes, uint8."""
    return _planes_merge_against("planes_merge_diff", planes, base)


def _planes_split_against(entry: str, array, base) -> list:
    """planes_split_delta and planes_split_diff: the host split of ``array`` against ``base`` by hsrans_<entry>"""
    a, b = np.ascontiguousarray(array), np.ascontiguousarray(base)
    if a.itemsize != b.itemsize or a.size != b.size:
        raise HsransError(f"{entry}: the base has the array's item size and count", code=2)
    planes = [np.empty(a.size, np.uint8) for _ in range(a.itemsize)]
    ptrs = (_vp * max(len(planes), 1))(*[p.ctypes.data for p in planes])
    _check(getattr(load_library(), "hsrans_" + entry)(a.itemsize, a.ctypes.data if a.size else ptrs, b.ctypes.data if b.size else ptrs, a.size, ptrs),
           "hsrans_" + entry)
    return planes


def _planes_merge_against(entry: str, planes, base) -> np.ndarray:
    """planes_merge_delta and planes_merge_diff: the host merge of ``planes`` against ``base`` by hsrans_<entry>"""
    planes, b = [_u8(p) for p in planes], np.ascontiguousarray(base)
    if len(planes) != b.itemsize or any(p.size != b.size for p in planes):
        raise HsransError(f"{entry}: one plane per byte of the base's items, each of the base's item count", code=2)
    out = np.empty(b.size * b.itemsize, np.uint8)
    ptrs = (_vp * max(len(planes), 1))(*[p.ctypes.data for p in planes])
    _check(getattr(load_library(), "hsrans_" + entry)(b.itemsize, ptrs, b.ctypes.data if b.size else ptrs, b.size, out.ctypes.data if out.size else ptrs),
           "hsrans_" + entry)
    return out


def _base_of(entry: str, base, tensor, optional: bool = False):
    """(pointer, bytes) of a delta call's base: a contiguous CUDA tensor of ``tensor``'s element size and element count"""
    if base is None and optional:
        return None, 0
    if not (isinstance(base, torch.Tensor) and base.is_cuda and base.is_contiguous() and base.element_size() == tensor.element_size() and base.numel() == tensor.numel()):
        raise HsransError(f"{entry}: a base is a contiguous CUDA tensor of the tensor's element size and element count", code=2)
    return base.data_ptr(), base.numel() * base.element_size()


def planes_gather_workspace_bytes(itemsize: int, count: int, total_elements: int) -> int:
    """hsrans_planes_gather_workspace_bytes: a workspace that takes every decode_device_planes_gather of ``count`` ranges with
    ``total_elements`` elements in all: itemsize * up256(total_elements + 30 * count) (0: an item size that is not 2, 4 or 8)."""
    return int(load_library().hsrans_planes_gather_workspace_bytes(itemsize, count, total_elements))


def planes_gather_indirect_workspace_bytes(itemsize: int, max_count: int) -> int:
    """hsrans_planes_gather_indirect_workspace_bytes: the control workspace a decode_device_planes_gather_indirect of up to ``max_count``
    ranges needs (a multiple of 256; 0: an item size that is not 2, 4 or 8, or max_count * itemsize at or above 2^31)."""
    return int(load_library().hsrans_planes_gather_indirect_workspace_bytes(itemsize, max_count))


def planes_gather_tasks(ranges, elements: int, capacity: int | None = None) -> np.ndarray:
    """hsrans_planes_gather_tasks: the merge tasks ``ranges`` ((N, 3) uint64 or a list of (offset, length, dst_offset), in elements) of a
    tensor of ``elements`` elements are cut into, as an (M, 5) uint64 array of (src, work_pos, dst_delta modulo 2^64, lo, hi).  Pure host
    arithmetic; an empty array for invalid input.  ``capacity``: as gather_tasks."""
    L = load_library()
    arr = _ranges_array(ranges)
    n = L.hsrans_planes_gather_tasks(_p(arr) if arr.size else None, arr.shape[0], elements, None, 0)
    rows = n if capacity is None else min(n, capacity)
    out = np.zeros(rows, np.dtype([("src", "<u8"), ("work_pos", "<u8"), ("dst_delta", "<u8"), ("lo", "<u4"), ("hi", "<u4")]))
    if rows:
        L.hsrans_planes_gather_tasks(_p(arr), arr.shape[0], elements, _p(out), rows)
    return np.stack([out[n].astype(np.uint64) for n in out.dtype.names], axis=1) if rows else np.zeros((0, 5), np.uint64)


def planes_gather_batch_workspace_bytes(max_itemsize: int, count: int, total_elements: int) -> int:
    """hsrans_planes_gather_batch_workspace_bytes: a workspace that takes every decode_device_planes_gather_batch of ``count`` rows with
    ``total_elements`` elements in all over members of at most ``max_itemsize`` bytes an item:
    up256(max_itemsize * (total_elements + 30 * count)) (0: an item size that is not 2, 4 or 8, or an overflow)."""
    return int(load_library().hsrans_planes_gather_batch_workspace_bytes(max_itemsize, count, total_elements))


def planes_gather_batch_indirect_workspace_bytes(coded_planes: int, max_itemsize: int, max_count: int) -> int:
    """hsrans_planes_gather_batch_indirect_workspace_bytes: the control workspace a decode_device_planes_gather_batch_indirect of up to
    ``max_count`` rows needs on a set with ``coded_planes`` coded planes in all (0: every plane stored) and members of at most
    ``max_itemsize`` bytes an element (0: another element size, more than 65,536 coded planes, or max_count * max_itemsize >= 2^31)"""
    return int(load_library().hsrans_planes_gather_batch_indirect_workspace_bytes(coded_planes, max_itemsize, max_count))


def planes_gather_batch_tasks(rows, itemsizes, elements, capacity: int | None = None) -> np.ndarray:
    """hsrans_planes_gather_batch_tasks: the merge tasks ``rows`` ((member, offset, length, dst_offset), in the member's elements) over
    members of ``itemsizes[m]``-byte items and ``elements[m]`` elements are cut into, as an (M, 7) uint64 array of (src, work_pos,
    plane_step, dst_delta modulo 2^64, lo, hi, member).  Pure host arithmetic; an empty array for invalid input.  ``capacity``: as
    gather_tasks."""
    L = load_library()
    arr = _member_ranges_array(rows)
    sizes, elems = np.ascontiguousarray(itemsizes, np.uint32).reshape(-1), np.ascontiguousarray(elements, np.uint64).reshape(-1)
    if sizes.size != elems.size:
        raise ValueError("one item size and one element count per member")
    args = (_p(arr) if arr.size else None, arr.shape[0], _p(sizes) if sizes.size else None, _p(elems) if elems.size else None, sizes.size)
    n = L.hsrans_planes_gather_batch_tasks(*args, None, 0)
    got = n if capacity is None else min(n, capacity)
    out = np.zeros(got, np.dtype([("src", "<u8"), ("work_pos", "<u8"), ("plane_step", "<u8"), ("dst_delta", "<u8"), ("lo", "<u4"), ("hi", "<u4"), ("member", "<u4"),
                                  ("reserved", "<u4")]))
    if got:
        L.hsrans_planes_gather_batch_tasks(*args, _p(out), got)
    return np.stack([out[n].astype(np.uint64) for n in out.dtype.names[:7]], axis=1) if got else np.zeros((0, 7), np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
class _Handle:
    """The owner of one C handle (``handle``, made by the library ``ctx.L``): ``_destroy`` names the C function that frees it.  close()
    frees it once, however often it is called; an object with ``owned`` False frees nothing; __del__ closes and swallows every error."""
    _destroy = ""
    handle = None  # (until __init__ has one: a constructor that raised leaves nothing to free)
    owned = True

    def _library(self):
        return self.ctx.L

    def close(self):
        h, self.handle = self.handle, None
        if h and self.owned:
            getattr(self._library(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch(_Handle):
    """hsrans_batch: K device plans decoded by one launch (Context.make_batch / Context.decode_device_batch)."""
    _destroy = "hsrans_dplan_batch_destroy"

    def __init__(self, ctx: "Context", handle, dplans):
        self.ctx, self.handle, self.dplans = ctx, handle, list(dplans)  # (keeps the member plans alive)

    def info(self) -> dict:
        info = BatchInfo()
        load_library().hsrans_dplan_batch_info(self.handle, ctypes.byref(info))
        return _as_dict(info)

    def read_finish(self) -> np.ndarray:
        out = np.zeros(1 << 16, np.uint64)
        n = load_library().hsrans_dplan_batch_read_finish(self.handle, _p(out), out.size)
        return out[:n].copy()


class Planes(_Handle):
    """hsrans_planes: a frame's descriptor bound to its planes' device plans (Context.make_planes / Context.decode_device_planes)."""
    _destroy = "hsrans_planes_destroy"

    def __init__(self, ctx: "Context", handle, desc: PlanesDesc, plans):
        self.ctx, self.handle, self.desc, self.plans = ctx, handle, desc, list(plans)  # (keeps the planes' plans alive)

    def info(self) -> dict:
        info = PlanesInfo()
        load_library().hsrans_planes_info(self.handle, ctypes.byref(info))
        return _as_dict(info)


class PlanesSet(_Handle):
    """hsrans_planes_set: many frames' descriptors bound to their planes' device plans (Context.make_planes_set /
    Context.decode_device_planes_batch)."""
    _destroy = "hsrans_planes_set_destroy"

    def __init__(self, ctx: "Context", handle, descs, plans_lists):
        self.ctx, self.handle, self.descs, self.plans = ctx, handle, list(descs), [list(p) for p in plans_lists]  # (keeps the planes' plans alive)

    def info(self) -> dict:
        """members; coded and stored planes of all members; the kernels of one decode (the batch's launches + the merge); the merge's
        workgroups; the workspace a decode needs"""
        info = PlanesSetInfo()
        load_library().hsrans_planes_set_info(self.handle, ctypes.byref(info))
        d = _as_dict(info)
        del d["reserved"]
        return d


class PlanesGather(_Handle):
    """hsrans_planes_gather: a Planes object bound to the frame it reads (Context.make_planes_gather / Context.decode_device_planes_gather)."""
    _destroy = "hsrans_planes_gather_destroy"

    def __init__(self, ctx: "Context", handle, planes: Planes, d_frame):
        self.ctx, self.handle, self.planes, self.d_frame = ctx, handle, planes, d_frame  # (keeps the planes object and the frame alive)

    def info(self) -> dict:
        """coded and stored planes, and of the last call: the gather's rows, the merge's tasks and the kernels launched"""
        info = PlanesGatherInfo()
        load_library().hsrans_planes_gather_info(self.handle, ctypes.byref(info))
        return _as_dict(info)

    def indirect_info(self, max_count: int, max_elements: int, out_capacity: int) -> dict:
        """hsrans_planes_gather_indirect_info: what a decode_device_planes_gather_indirect of up to ``max_count`` ranges and ``max_elements``
        elements will launch — coded and stored planes, the set's rows at most, the merge's grid, all kernels of a call and the set's part
        of them.  No device call."""
        info = PlanesGatherIndirectInfo()
        _check(load_library().hsrans_planes_gather_indirect_info(self.handle, max_count, max_elements, out_capacity, ctypes.byref(info)),
               "hsrans_planes_gather_indirect_info")
        return _as_dict(info)


class PlanesGatherSet(_Handle):
    """hsrans_planes_gather_set: a PlanesSet bound to the frames it reads (Context.make_planes_gather_set /
    Context.decode_device_planes_gather_batch)."""
    _destroy = "hsrans_planes_gather_set_destroy"

    def __init__(self, ctx: "Context", handle, pset: PlanesSet, d_frames):
        self.ctx, self.handle, self.pset, self.d_frames = ctx, handle, pset, list(d_frames)  # (keeps the planes set and the frames alive)
        # what sizes the indirect call's control workspace: the coded planes of all members and the largest element size
        self.coded = sum(p is not None for plans in pset.plans for p in plans)
        self.max_itemsize = max((int(d.elem_size) for d in pset.descs), default=0)

    def info(self) -> dict:
        """members, coded and stored planes of all members, and of the last call: the gather's rows, the merge's tasks and the kernels launched"""
        info = PlanesGatherSetInfo()
        load_library().hsrans_planes_gather_set_info(self.handle, ctypes.byref(info))
        return _as_dict(info)

    def indirect_info(self, max_count: int, out_capacity: int, work_bytes: int) -> dict:
        """hsrans_planes_gather_set_indirect_info: what a decode_device_planes_gather_batch_indirect of up to ``max_count`` rows with a data
        workspace of ``work_bytes`` will launch — members, coded and stored planes, the set's rows at most, the merge's grid, all kernels of
        a call and the set's part of them.  No device call."""
        info = PlanesGatherSetIndirectInfo()
        _check(load_library().hsrans_planes_gather_set_indirect_info(self.handle, max_count, out_capacity, work_bytes, ctypes.byref(info)),
               "hsrans_planes_gather_set_indirect_info")
        return _as_dict(info)


class PlanesBaseSet(_Handle):
    """hsrans_planes_base_set: one base (or None) per member of a PlanesGatherSet, for decode_device_planes_gather_batch_delta and
    decode_device_planes_gather_batch_indirect_delta (Context.make_planes_base_set).  Close it before its gather set."""
    _destroy = "hsrans_planes_base_set_destroy"

    def __init__(self, ctx: "Context", handle, pgs: PlanesGatherSet, bases):
        self.ctx, self.handle, self.pgs, self.bases = ctx, handle, pgs, list(bases)  # (keeps the gather set and the bases alive)


class GatherSet(_Handle):
    """hsrans_gather_set: K device plans bound to their compressed streams (Context.make_gather_set / Context.decode_device_gather_batch)."""
    _destroy = "hsrans_gather_set_destroy"

    def __init__(self, ctx: "Context", handle, dplans, d_streams):
        self.ctx, self.handle, self.dplans, self.d_streams = ctx, handle, list(dplans), list(d_streams)  # (keeps the plans and the streams alive)

    def info(self) -> dict:
        """members, members per kind, and of the last gather: launches and per kind tasks, entries (tasks + padding), grid, waves, LDS bytes"""
        info = GatherSetInfo()
        load_library().hsrans_gather_set_info(self.handle, ctypes.byref(info))
        return _as_dict(info)

    def indirect_info(self, max_count: int, dst_capacity: int) -> dict:
        """hsrans_gather_set_indirect_info: what a decode_device_gather_batch_indirect of up to ``max_count`` ranges into ``dst_capacity``
        bytes will launch — members, members per kind, the launches behind the cut and per kind grid, waves and LDS bytes (tasks and
        entries are 0: only the device knows them).  Pure host arithmetic."""
        info = GatherSetInfo()
        _check(load_library().hsrans_gather_set_indirect_info(self.handle, max_count, dst_capacity, ctypes.byref(info)), "hsrans_gather_set_indirect_info")
        return _as_dict(info)


class DevicePlan(_Handle):
    _destroy = "hsrans_dplan_destroy"

    def __init__(self, ctx: "Context", handle, owned: bool = True):
        self.ctx, self.handle, self.owned = ctx, handle, owned  # (owned False: a view of a plan another object destroys, e.g. a Sharded's sub-run)

    def launch_info(self) -> dict:
        info = LaunchInfo()
        load_library().hsrans_dplan_launch_info(self.handle, ctypes.byref(info))
        return _as_dict(info)


class Comm(_Handle):
    """hsrans_comm: this process's rank in a communicator over the GPUs of the node (RCCL, bound by the C library at run time)."""
    _destroy = "hsrans_comm_destroy"

    def __init__(self, ctx: "Context", comm_id: bytes, rank: int, world: int):
        assert len(comm_id) == COMM_ID_BYTES
        self.ctx = ctx
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(comm_id)
        h = _vp()
        _check(ctx.L.hsrans_comm_create(ctx.handle, buf, rank, world, ctypes.byref(h)), f"hsrans_comm_create(rank {rank} of {world})")
        self.handle, self.rank, self.world = h, rank, world

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
        _check(load_library().hsrans_comm_unique_id(buf), "hsrans_comm_unique_id", " (no RCCL could be bound?)")
        return bytes(buf)


class Queue(_Handle):
    """hsrans_queue: streams submitted one by one, decoded by ONE batch launch per flush (the dealing cached per shape)."""
    _destroy = "hsrans_queue_destroy"

    def __init__(self, ctx: "Context", max_members: int = 32):
        self.ctx = ctx
        h = _vp()
        _check(ctx.L.hsrans_queue_create(ctx.handle, max_members, ctypes.byref(h)), "hsrans_queue_create")
        self.handle = h
        self._keep = []  # tensors and plans of the submissions still pending

    def submit(self, dplan: "DevicePlan", d_stream: torch.Tensor, d_out: torch.Tensor, stream_length: int | None = None, stream: torch.cuda.Stream | None = None):
        _check(self.ctx.L.hsrans_queue_submit(self.handle, dplan.handle, d_stream.data_ptr(), d_stream.numel() if stream_length is None else stream_length,
                                              d_out.data_ptr(), d_out.numel(), _stream(stream, d_out.device)), "hsrans_queue_submit")
        self._keep.append((dplan, d_stream, d_out))
        if self.pending() == 0:
            self._keep.clear()

    def flush(self, stream: torch.cuda.Stream | None = None):
        rc = self.ctx.L.hsrans_queue_flush(self.handle, _stream(stream))
        self._keep.clear()
        _check(rc, "hsrans_queue_flush")

    def pending(self) -> int:
        return int(self.ctx.L.hsrans_queue_pending(self.handle))

    def stats(self) -> dict:
        st = QueueStats()
        self.ctx.L.hsrans_queue_stats(self.handle, ctypes.byref(st))
        return _as_dict(st)  # (uint64 fields: Python ints)


class Sharded(_Handle):
    """hsrans_sharded: this rank's share of ONE stream decoded by all ranks of a communicator (or, without one, decode only)."""
    _destroy = "hsrans_sharded_destroy"

    def __init__(self, ctx: "Context", plan, parts: int = 1, weights=None, root: int | None = None, comm: Comm | None = None, rank: int | None = None,
                 world: int | None = None):
        plan = _u8(plan)
        self.ctx, self.comm = ctx, comm
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        h = _vp()
        r = -1 if root is None else int(root)
        if comm is not None:
            rc = ctx.L.hsrans_sharded_create(ctx.handle, comm.handle, _p(plan), plan.size, parts, None if w is None else _p(w), r, ctypes.byref(h))
        else:
            rc = ctx.L.hsrans_sharded_create_rank(ctx.handle, rank, world, _p(plan), plan.size, parts, None if w is None else _p(w), r, ctypes.byref(h))
        _check(rc, "hsrans_sharded_create")
        self.handle = h
        info = ShardedInfo()
        shards = (Shard * (int(world if comm is None else comm.world) * parts))()
        ctx.L.hsrans_sharded_info(h, ctypes.byref(info), shards, len(shards))
        self.info = _as_dict(info)
        self.shards = [[(int(shards[q * parts + k].first_chain), int(shards[q * parts + k].chain_count), int(shards[q * parts + k].out_begin), int(shards[q * parts + k].out_end))
                        for k in range(parts)] for q in range(info.world)]

    def part_plan(self, k: int) -> DevicePlan | None:
        h = self.ctx.L.hsrans_sharded_part_plan(self.handle, k)
        return DevicePlan(self.ctx, _vp(h), owned=False) if h else None

    def wait_part(self, part: int, stream: torch.cuda.Stream):
        """hsrans_sharded_wait_part: `stream` waits until sub-run `part` of the last decode() is complete and visible"""
        _check(self.ctx.L.hsrans_sharded_wait_part(self.handle, part, _vp(stream.cuda_stream)), "hsrans_sharded_wait_part")

    def whole_plan(self) -> DevicePlan | None:
        """this rank's whole run when ONE launch decodes all its sub-runs (hsrans_sharded_info: one_launch), else None"""
        h = self.ctx.L.hsrans_sharded_whole_plan(self.handle)
        return DevicePlan(self.ctx, _vp(h), owned=False) if h else None

    def decode(self, d_window: torch.Tensor, d_out: torch.Tensor, mode: int = SHARD_DECODE_AND_EXCHANGE, stream: torch.cuda.Stream | None = None):
        _check(self.ctx.L.hsrans_decode_sharded(self.handle, d_window.data_ptr(), d_out.data_ptr(), mode, _stream(stream, d_out.device)), "hsrans_decode_sharded")

    def status(self, stream: torch.cuda.Stream | None = None) -> int:
        return self.ctx.L.hsrans_sharded_status(self.handle, _stream(stream))


def _calibration_report(rep: Calibration) -> dict:
    return {"class_weights": list(rep.class_weights), "class_finish_us_last_iteration": [round(v, 3) for v in rep.class_finish_us_last_iteration],
            "last_wave_us_before": rep.last_wave_us_before, "last_wave_us_after": rep.last_wave_us_after,
            "class_spread_us_before": rep.class_spread_us_before, "class_spread_us_after": rep.class_spread_us_after,
            "iterations": rep.iterations, "bytes": rep.bytes}


class Context(_Handle):
    """hsrans_ctx: one per GPU.  Raises if no gfx950 device is usable (there is no CPU decode path)."""
    _destroy = "hsrans_ctx_destroy"

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = _vp()
        _check(self.L.hsrans_ctx_create(device, ctypes.byref(h)), f"hsrans_ctx_create(device={device})", ": a gfx950 GPU is required")
        self.handle = h
        self.device = device

    def _library(self):
        return self.L

    @property
    def device_name(self) -> str:
        return self.L.hsrans_ctx_device_name(self.handle).decode()

    def calibrate(self, bits: int = 11, iterations: int = 0) -> dict:
        """hsrans_ctx_calibrate: fits the one-chain-per-wave index's class lengths to this device; returns the report."""
        rep = Calibration()
        _check(self.L.hsrans_ctx_calibrate(self.handle, bits, iterations, ctypes.byref(rep)), "hsrans_ctx_calibrate")
        return _calibration_report(rep)

    def calibrate_runs(self, bits: int = 11, copies: int = 2, iterations: int = 0) -> dict:
        """hsrans_ctx_calibrate_runs: the same fit for runs ``copies`` times as long (``copies`` members of the calibration stream in one launch)."""
        rep = Calibration()
        _check(self.L.hsrans_ctx_calibrate_runs(self.handle, bits, iterations, copies, ctypes.byref(rep)), "hsrans_ctx_calibrate_runs")
        return {"copies": copies, **_calibration_report(rep)}

    # -- host-pointer drop-in: decodeFunc(pInData, inLength, pOutData, outCapacity) ------------------------------
    def decode_host(self, container: int, states: int, bits: int, stream, out_capacity: int, plan=None, in_length: int | None = None):
        """Returns (returned_length, out) like the reference's decoders: returned_length == 0 means failure."""
        stream = _u8(stream)
        out = np.full(max(out_capacity, 1), 0xCC, np.uint8)
        pp, pn = (None, 0)
        if plan is not None:
            plan = _u8(plan)
            pp, pn = _p(plan), plan.size
        r = self.L.hsrans_decode_host(self.handle, container, states, bits, _p(stream), stream.size if in_length is None else in_length, _p(out),
                                      out_capacity, pp, pn)
        return r, out[:out_capacity]

    def host_index_chains(self) -> int:
        """chains of the index decode_host keeps from its last plan-less call on an mt_, block_ or raw stream of >= 1 MiB (0 = none)"""
        return int(self.L.hsrans_ctx_host_index_chains(self.handle))

    def decode(self, container: int, states: int, bits: int, stream, plan=None) -> np.ndarray:
        stream = _u8(stream)
        n = int(stream[:8].view(np.uint64)[0]) if stream.size >= 8 else 0
        r, out = self.decode_host(container, states, bits, stream, n, plan)
        if r == 0:
            raise HsransError("decode failed (malformed stream or no device)")
        return out[:r]

    # -- device-resident path ------------------------------------------------------------------------------------
    def make_device_plan(self, plan) -> DevicePlan:
        plan = _u8(plan)
        h = _vp()
        _check(self.L.hsrans_dplan_create(self.handle, _p(plan), plan.size, ctypes.byref(h)), "hsrans_dplan_create")
        return DevicePlan(self, h)

    def make_device_plan_from_stream(self, container: int, states: int, bits: int, d_stream: torch.Tensor, stream_length: int,
                                     out_capacity: int, stream: torch.cuda.Stream | None = None) -> DevicePlan:
        """A plan for a stream that only exists in device memory.  mt_: the header chain is walked on the GPU.  block_: the walk plan
        (one wavefront follows the inline headers), made from the stream's first 16 + 4 * states bytes; :meth:`decode_device_indexing`
        turns it into a plan with checkpoints.  Raw streams are refused (plan_build needs their header only)."""
        h = _vp()
        _check(self.L.hsrans_dplan_create_from_device_stream(self.handle, container, states, bits, d_stream.data_ptr(), stream_length, out_capacity,
                                                             _stream(stream, d_stream.device), ctypes.byref(h)), "hsrans_dplan_create_from_device_stream")
        return DevicePlan(self, h)

    def read_device_plan(self, dplan: DevicePlan, capacity: int = 1 << 28) -> np.ndarray:
        out = np.zeros(capacity, np.uint8)
        n = self.L.hsrans_dplan_read_plan(dplan.handle, _p(out), out.size)
        if n == 0:
            raise HsransError("hsrans_dplan_read_plan failed")
        return out[:n].copy()

    def decode_device(self, dplan: DevicePlan, d_stream: torch.Tensor, d_out: torch.Tensor, stream: torch.cuda.Stream | None = None,
                      stream_length: int | None = None):
        """Asynchronous launch on ``stream`` (default: torch's current stream).  Tensors are uint8, on this context's GPU."""
        _check(self.L.hsrans_decode_device(self.handle, dplan.handle, d_stream.data_ptr(), d_stream.numel() if stream_length is None else stream_length,
                                           d_out.data_ptr(), d_out.numel(), _stream(stream, d_stream.device)), "hsrans_decode_device")

    def decode_device_indexing(self, dplan: DevicePlan, d_stream: torch.Tensor, d_out: torch.Tensor, index_interval: int,
                               stream: torch.cuda.Stream | None = None, stream_length: int | None = None) -> DevicePlan:
        """First decode of a stream without an index: fills ``d_out`` and returns the plan with a checkpoint every
        ``index_interval`` groups for the later decodes (hsrans_decode_device_indexing; synchronises ``stream``).  ``dplan``: a raw or mt_
        base plan, or a block_ stream's walk plan (``make_device_plan_from_stream(BLOCK, ...)`` or ``make_device_plan(plan_build(BLOCK, ...))``).
        Raises HsransError; for a block_ stream with more than ``decoded_len / 4096 + 16`` blocks (code 3) ``d_out`` is complete all the same."""
        h = _vp()
        _check(self.L.hsrans_decode_device_indexing(self.handle, dplan.handle, d_stream.data_ptr(), d_stream.numel() if stream_length is None else stream_length,
                                                    d_out.data_ptr(), d_out.numel(), index_interval, _stream(stream, d_stream.device), ctypes.byref(h)),
               "hsrans_decode_device_indexing")
        return DevicePlan(self, h)

    def decode_device_indexing_batch(self, members, stream: torch.cuda.Stream | None = None, stats: dict | None = None):
        """The first decode of many streams in one call (hsrans_decode_device_indexing_batch): member k is ``(dplan, d_stream, d_out,
        index_interval)`` or ``(dplan, d_stream, d_out, index_interval, stream_length)`` — a block_ stream's walk plan or an mt_ base
        plan, uint8 CUDA tensors on one device — and gets what :meth:`decode_device_indexing` gives it.  Returns the list of indexed
        DevicePlans.  ``stats``: filled with hsrans_indexing_batch_stats.  Raises HsransError when any member failed; the error
        carries ``code``, ``codes`` (per member) and ``plans`` (a DevicePlan or None per member: what the members that did not
        fail got).  Synchronises ``stream``."""
        members = list(members)
        dev = None
        for k, m in enumerate(members):
            if not isinstance(m, (tuple, list)) or len(m) not in (4, 5):
                raise TypeError(f"decode_device_indexing_batch: member {k}: (dplan, d_stream, d_out, index_interval[, stream_length]) expected")
            if not isinstance(m[0], DevicePlan):
                raise TypeError(f"decode_device_indexing_batch: member {k}: a DevicePlan expected")
            for name, t in (("d_stream", m[1]), ("d_out", m[2])):
                if not getattr(t, "is_cuda", False) or t.dtype != torch.uint8 or not t.is_contiguous():
                    raise TypeError(f"decode_device_indexing_batch: member {k}: {name} must be a contiguous uint8 CUDA tensor")
                dev = t.device if dev is None else dev
                if t.device != dev:
                    raise TypeError(f"decode_device_indexing_batch: member {k}: {name} is on {t.device}, the others on {dev}")
            if not isinstance(m[3], int) or (len(m) == 5 and not isinstance(m[4], int)):
                raise TypeError(f"decode_device_indexing_batch: member {k}: index_interval and stream_length are integers")
        K = len(members)
        arr = (IndexingMember * max(K, 1))()
        for k, m in enumerate(members):
            e = arr[k]
            e.dplan, e.d_stream, e.d_out, e.index_interval = m[0].handle, m[1].data_ptr(), m[2].data_ptr(), m[3]
            e.stream_length, e.out_capacity = (m[4] if len(m) == 5 else m[1].numel()), m[2].numel()
        st = IndexingBatchStats()
        rc = self.L.hsrans_decode_device_indexing_batch(self.handle, arr, K, _stream(stream, dev), ctypes.byref(st))
        if stats is not None:
            stats.update(_as_dict(st))
        if K == 0:
            _check(rc, "hsrans_decode_device_indexing_batch")
        codes = [int(arr[k].rc) for k in range(K)]
        plans = [DevicePlan(self, _vp(arr[k].indexed)) if arr[k].indexed else None for k in range(K)]
        if rc != 0:
            failed = [] if rc in (2, 4) else [k for k in range(K) if codes[k] != 0]  # (2, 4: the call as a whole was refused)
            raise _members_error("hsrans_decode_device_indexing_batch", rc, failed, codes=codes, plans=plans)
        return plans

    def decode_device_window(self, dplan: DevicePlan, d_window: torch.Tensor, window_offset: int, window_length: int, d_out: torch.Tensor,
                             stream: torch.cuda.Stream | None = None):
        """As decode_device for a caller that holds only stream bytes [window_offset, window_offset + window_length) (hsrans_decode_device_window)."""
        _check(self.L.hsrans_decode_device_window(self.handle, dplan.handle, d_window.data_ptr(), window_offset, window_length, d_out.data_ptr(), d_out.numel(),
                                                  _stream(stream, d_window.device)), "hsrans_decode_device_window")

    def decode_device_ranges(self, dplan: DevicePlan, d_window: torch.Tensor, window_offset: int, window_length: int, d_out_window: torch.Tensor,
                             out_offset: int, out_length: int, stream: torch.cuda.Stream | None = None):
        """As decode_device_window for a caller that also holds only output bytes [out_offset, out_offset + out_length)
        (hsrans_decode_device_ranges): one rank's share of a sharded decode."""
        assert d_out_window.numel() >= out_length
        _check(self.L.hsrans_decode_device_ranges(self.handle, dplan.handle, d_window.data_ptr(), window_offset, window_length, d_out_window.data_ptr(),
                                                  out_offset, out_length, _stream(stream, d_window.device)), "hsrans_decode_device_ranges")

    def decode_device_gather(self, dplan: DevicePlan, d_stream: torch.Tensor, ranges, d_dst: torch.Tensor, stream_length: int | None = None,
                             stream: torch.cuda.Stream | None = None):
        """Byte ranges of a stream that stays compressed on the GPU, one launch (hsrans_decode_device_gather): for every row
        (offset, length, dst_offset) of ``ranges`` ((N, 3) uint64 or a list of triples) the decoded bytes [offset, offset + length) land at
        d_dst[dst_offset:]; no other byte of ``d_dst`` is written.  Asynchronous on ``stream`` (default: torch's current stream); ``ranges`` is
        read before the call returns.  Destinations that overlap are the caller's responsibility.  Raises HsransError (``.code``: 2 bad
        argument or range, 3 a plan without entry points or a wrong stream length)."""
        arr = _ranges_array(ranges)
        _check(self.L.hsrans_decode_device_gather(self.handle, dplan.handle, d_stream.data_ptr(), d_stream.numel() if stream_length is None else stream_length,
                                                  _p(arr) if arr.size else None, arr.shape[0], d_dst.data_ptr(), d_dst.numel(), _stream(stream, d_stream.device)),
               "hsrans_decode_device_gather")

    def decode_device_gather_indirect(self, dplan: DevicePlan, d_stream: torch.Tensor, d_ranges: torch.Tensor, d_dst: torch.Tensor, count: torch.Tensor | None = None,
                                      max_count: int | None = None, workspace: torch.Tensor | None = None, stream_length: int | None = None,
                                      stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """decode_device_gather for ranges that are on the GPU (hsrans_decode_device_gather_indirect): ``d_ranges`` is a contiguous CUDA
        tensor (N, 3) of int64 / uint64 rows (offset, length, dst_offset), ``count`` a CUDA int32 / uint32 scalar tensor with the number of
        rows in use (None: ``max_count``, itself N when None).  Both are read when the launch runs, not here: nothing is copied to the host,
        nothing is waited for, and the call can be captured into a graph.  ``workspace``: a CUDA uint8 tensor of at least
        gather_workspace_bytes(max_count) bytes that no other call in flight uses; allocated here when None.  Returns the workspace.
        Raises HsransError (``.code``) for what the host can check; a range or count only the device can refuse leaves ``d_dst`` untouched
        and is reported by ``status(dplan)`` (5)."""
        max_count, workspace = _indirect_args(d_ranges, 3, count, max_count, workspace, gather_workspace_bytes, d_stream.device, stream)
        _check(self.L.hsrans_decode_device_gather_indirect(self.handle, dplan.handle, d_stream.data_ptr(), d_stream.numel() if stream_length is None else stream_length,
                                                           d_ranges.data_ptr(), None if count is None else count.data_ptr(), max_count, d_dst.data_ptr(), d_dst.numel(),
                                                           workspace.data_ptr(), workspace.numel(), _stream(stream, d_stream.device)),
               "hsrans_decode_device_gather_indirect")
        return workspace

    def make_gather_set(self, dplans, d_streams, stream_lengths=None) -> GatherSet:
        """Binds K device plans to their streams (hsrans_gather_set_create): member k = dplans[k] over the CUDA uint8 tensor d_streams[k]
        (16-byte aligned; ``stream_lengths[k]`` bytes of it, default all).  The set keeps the plans and the tensors alive.  Raises HsransError
        (``.code``: 2 a bad argument or a misaligned stream, 3 a plan without entry points or a wrong stream length)."""
        dplans, d_streams = list(dplans), list(d_streams)
        K = len(dplans)
        if len(d_streams) != K:
            raise ValueError("one stream per device plan")
        sp, sl = _tensor_arrays(d_streams, stream_lengths)
        h = _vp()
        _check(self.L.hsrans_gather_set_create(self.handle, _handle_array(dplans), sp, sl, K, ctypes.byref(h)), "hsrans_gather_set_create")
        return GatherSet(self, h, dplans, d_streams)

    def decode_device_gather_batch(self, gset: GatherSet, ranges, d_dst: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """Byte ranges of many streams that stay compressed on the GPU, one launch per table layout (hsrans_decode_device_gather_batch): for
        every row (member, offset, length, dst_offset) of ``ranges`` ((N, 4) uint64 or a list of such rows) the decoded bytes
        [offset, offset + length) of that member land at d_dst[dst_offset:]; no other byte of ``d_dst`` is written — byte for byte what one
        decode_device_gather per member gives.  Asynchronous on ``stream`` (default: torch's current stream); ``ranges`` is read before the
        call returns.  Raises HsransError (``.code``: 2 a bad member, range or destination; nothing was launched)."""
        arr = _member_ranges_array(ranges)
        _check(self.L.hsrans_decode_device_gather_batch(self.handle, gset.handle, _p(arr) if arr.size else None, arr.shape[0], d_dst.data_ptr(), d_dst.numel(),
                                                        _stream(stream, d_dst.device)), "hsrans_decode_device_gather_batch")

    def decode_device_gather_batch_indirect(self, gset: GatherSet, d_ranges: torch.Tensor, d_dst: torch.Tensor, count: torch.Tensor | None = None,
                                            max_count: int | None = None, workspace: torch.Tensor | None = None,
                                            stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """decode_device_gather_batch for ranges that are on the GPU (hsrans_decode_device_gather_batch_indirect): ``d_ranges`` is a
        contiguous CUDA tensor (N, 4) of int64 / uint64 rows (offset, length, dst_offset, member) — the memory layout of
        hsrans_member_range: ``member`` is the low 32 bits of the fourth column, the high 32 bits are ``reserved`` and must be 0 —
        ``count`` a CUDA int32 / uint32 scalar tensor with the number of rows in use (None: ``max_count``, itself N when None).  Both are
        read when the launches run, not here: nothing is copied to the host, nothing is waited for, and the call can be captured into a
        graph.  ``workspace``: a CUDA uint8 tensor of at least gather_batch_workspace_bytes(members, max_count) bytes that no other call in
        flight uses; allocated here when None.  Returns the workspace.  Raises HsransError (``.code``) for what the host can check; a row or
        count only the device can refuse leaves ``d_dst`` untouched and is reported by ``gather_set_refused(gset)`` (5)."""
        max_count, workspace = _indirect_args(d_ranges, 4, count, max_count, workspace, lambda n: gather_batch_workspace_bytes(len(gset.dplans), n), d_dst.device,
                                              stream)
        _check(self.L.hsrans_decode_device_gather_batch_indirect(self.handle, gset.handle, d_ranges.data_ptr(), None if count is None else count.data_ptr(), max_count,
                                                                 d_dst.data_ptr(), d_dst.numel(), workspace.data_ptr(), workspace.numel(), _stream(stream, d_dst.device)),
               "hsrans_decode_device_gather_batch_indirect")
        return workspace

    def gather_set_refused(self, gset: GatherSet, stream: torch.cuda.Stream | None = None) -> int:
        """hsrans_gather_set_refused: synchronises ``stream`` and returns 5 once where a decode_device_gather_batch_indirect on the set was
        refused on the device since the last look, else 0"""
        return int(self.L.hsrans_gather_set_refused(self.handle, gset.handle, _stream(stream)))

    def gather_set_status(self, gset: GatherSet, stream: torch.cuda.Stream | None = None) -> list:
        """hsrans_gather_set_status: synchronises ``stream`` and returns every member's status (0, or 5: its kernel found a malformed histogram)"""
        codes = (ctypes.c_int * len(gset.dplans))()
        self.L.hsrans_gather_set_status(self.handle, gset.handle, _stream(stream), codes)
        return list(codes)

    # -- K independent streams, one launch -------------------------------------------------------------------------
    def make_batch(self, dplans) -> Batch:
        dplans = list(dplans)
        h = _vp()
        _check(self.L.hsrans_dplan_batch_create(self.handle, _handle_array(dplans), len(dplans), ctypes.byref(h)), "hsrans_dplan_batch_create")
        return Batch(self, h, dplans)

    def decode_device_batch(self, batch: Batch, d_streams, d_outs, stream: torch.cuda.Stream | None = None, stream_lengths=None):
        """Asynchronous on ``stream`` (default: torch's current stream): member k decodes d_streams[k] into d_outs[k]."""
        K = len(batch.dplans)
        assert len(d_streams) == K and len(d_outs) == K
        sp, sl = _tensor_arrays(d_streams, stream_lengths)
        op, oc = _tensor_arrays(d_outs)
        _check(self.L.hsrans_decode_device_batch(self.handle, batch.handle, sp, sl, op, oc, _stream(stream, d_streams[0].device)), "hsrans_decode_device_batch")

    def batch_status(self, batch: Batch, stream: torch.cuda.Stream | None = None) -> list:
        codes = (ctypes.c_int * len(batch.dplans))()
        self.L.hsrans_dplan_batch_status(self.handle, batch.handle, _stream(stream), codes)
        return list(codes)

    def status(self, dplan: DevicePlan, stream: torch.cuda.Stream | None = None) -> int:
        return self.L.hsrans_dplan_status(self.handle, dplan.handle, _stream(stream))

    def encode_device(self, container: int, states: int, bits: int, d_in: torch.Tensor, d_out: torch.Tensor, block_size: int = 1 << 16,
                      index_interval: int = 0, want_plan: bool = False, stream: torch.cuda.Stream | None = None):
        """GPU encoder (mt_, independent fixed-size blocks).  Returns the stream length written to d_out, or
        ``(length, DevicePlan)`` with ``want_plan`` (plan with a checkpoint every ``index_interval`` groups, built on the device)."""
        h = _vp()
        n = self.L.hsrans_encode_device(self.handle, container, states, bits, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(), block_size,
                                        index_interval, _stream(stream, d_in.device), ctypes.byref(h) if want_plan else None)
        if n == 0:
            raise HsransError("hsrans_encode_device failed")
        return (n, DevicePlan(self, h)) if want_plan else n

    def encode_device_raw(self, states: int, bits: int, d_in: torch.Tensor, d_out: torch.Tensor, hist=None, index_interval: int = 0, index_groups=None,
                          want_plan: bool = False, want_device_plan: bool = False, stream: torch.cuda.Stream | None = None):
        """GPU encoder for the raw format (one wavefront: hsrans_encode_device_raw).  Returns the stream length, followed by the plan
        blob (``want_plan``) and/or a DevicePlan (``want_device_plan``) when an index (``index_interval`` or ``index_groups``) is asked for."""
        groups = np.ascontiguousarray(index_groups, dtype=np.uint64) if index_groups is not None else None
        n_groups = 0 if groups is None else groups.size
        plan, psize, h = None, _sz(0), _vp()
        if want_plan:
            pcap = (self.L.hsrans_plan_capacity_chains(RAW, states, d_in.numel(), n_groups, 0) if n_groups
                    else self.L.hsrans_plan_capacity(RAW, states, d_in.numel(), index_interval, 0))
            plan = np.zeros(pcap, np.uint8)
        n = self.L.hsrans_encode_device_raw(self.handle, states, bits, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(),
                                            ctypes.addressof(hist) if hist is not None else None, index_interval, _p(groups) if n_groups else None, n_groups,
                                            _p(plan) if want_plan else None, plan.size if want_plan else 0, ctypes.byref(psize),
                                            _stream(stream, d_in.device), ctypes.byref(h) if want_device_plan else None)
        if n == 0:
            raise HsransError("hsrans_encode_device_raw failed")
        out = [n]
        if want_plan:
            out.append(plan[: psize.value].copy())
        if want_device_plan:
            out.append(DevicePlan(self, h))
        return out[0] if len(out) == 1 else tuple(out)

    def encode_device_ex(self, container: int, states: int, bits: int, d_in: torch.Tensor, d_out: torch.Tensor, hist=None, block_size: int = 0,
                         independent_blocks: bool = False, index_interval: int = 0, index_groups=None, want_plan: bool = False,
                         want_device_plan: bool = False, stream: torch.cuda.Stream | None = None):
        """GPU twin of :func:`encode` (hsrans_encode_device_ex): every container, the adaptive (``block_size=0``) or fixed blocks, the
        same stream bytes and plan.  Returns the stream length, followed by the plan blob (``want_plan``) and/or a DevicePlan
        (``want_device_plan``) when an index (``index_interval`` or ``index_groups``) is asked for."""
        groups = np.ascontiguousarray(index_groups, dtype=np.uint64) if index_groups is not None else None
        if groups is not None and groups.size == 0:  # a stream too short for more than one chain (as encode())
            groups, index_interval = None, 4
        n_groups = 0 if groups is None else groups.size
        indexed = index_interval != 0 or n_groups != 0
        plan = np.zeros(1, np.uint8)
        if indexed:
            pcap = (self.L.hsrans_plan_capacity_chains(container, states, d_in.numel(), n_groups, block_size) if n_groups
                    else self.L.hsrans_plan_capacity(container, states, d_in.numel(), index_interval, block_size))
            plan = np.zeros(max(pcap, 1), np.uint8)
        opts = EncodeOpts(block_size, 0 if n_groups else index_interval, plan.ctypes.data if indexed else None, plan.size if indexed else 0, 0,
                          ENC_INDEPENDENT_BLOCKS if independent_blocks else 0, 0, groups.ctypes.data if n_groups else None, n_groups)
        h = _vp()
        n = self.L.hsrans_encode_device_ex(self.handle, container, states, bits, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(),
                                           ctypes.byref(hist) if hist is not None else None, ctypes.byref(opts), _stream(stream, d_in.device),
                                           ctypes.byref(h) if want_device_plan and indexed else None)
        if n == 0:
            raise HsransError("hsrans_encode_device_ex failed")
        out = [n]
        if want_plan and indexed:
            out.append(plan[: opts.plan_size].copy())
        if want_device_plan and indexed:
            out.append(DevicePlan(self, h))
        return out[0] if len(out) == 1 else tuple(out)

    def encode_device_batch(self, members, want_plans: bool = False, stream: torch.cuda.Stream | None = None, stats: dict | None = None):
        """Many streams in one call (hsrans_encode_device_batch): member k is ``(container, states, bits, d_in, d_out)`` or
        ``(container, states, bits, d_in, d_out, options)`` with ``options`` a dict of ``block_size`` (mt_; default 2^16),
        ``index_interval``, ``hist`` (raw: a Hist), ``index_groups`` (raw) and ``length`` (default ``d_in.numel()``).  Each member gets
        what its single call (``encode_device_raw`` / ``encode_device``) gives.  Returns the stream lengths, or ``(lengths, plans)``
        with ``want_plans`` (a DevicePlan or None per member: raw members have one only with an index).  ``stats``: filled with
        hsrans_encode_batch_stats.  Raises HsransError naming the first failed member; the error carries ``code``, ``lengths``
        and ``plans`` (what the members that did not fail got)."""
        K = len(members)
        arr = (EncodeMember * max(K, 1))()
        keep = []  # (the hists and group lists must outlive the call)
        dev = None
        for k, m in enumerate(members):
            container, states, bits, d_in, d_out, o = _encode_member("encode_device_batch", k, m, ("block_size", "index_interval", "hist", "index_groups", "length"))
            dev = d_in.device if dev is None else dev
            e = arr[k]
            e.container, e.states, e.bits = container, states, bits
            e.block_size = o.get("block_size", 1 << 16 if container == MT else 0)
            e.d_in, e.length = d_in.data_ptr(), int(o.get("length", d_in.numel()))
            e.d_out, e.out_capacity = d_out.data_ptr(), d_out.numel()
            e.index_interval = o.get("index_interval", 0)
            if o.get("hist") is not None:
                keep.append(o["hist"])
                e.hist = ctypes.addressof(o["hist"])
            if o.get("index_groups") is not None:
                g = np.ascontiguousarray(o["index_groups"], dtype=np.uint64)
                keep.append(g)
                e.index_groups, e.n_index_groups = (g.ctypes.data if g.size else None), g.size
        handles = (_vp * max(K, 1))()
        st = EncodeBatchStats()
        rc = self.L.hsrans_encode_device_batch(self.handle, arr, K, _stream(stream, dev), handles if want_plans else None, ctypes.byref(st))
        if stats is not None:
            stats.update(_as_dict(st))
        lengths = [int(arr[k].stream_length) for k in range(K)]
        plans = [DevicePlan(self, _vp(handles[k])) if want_plans and handles[k] else None for k in range(K)]
        if rc != 0:
            failed = [] if rc == 2 else [k for k in range(K) if lengths[k] == 0]  # (2: a check refused the call as a whole)
            raise _members_error("hsrans_encode_device_batch", rc, failed, lengths=lengths, plans=plans)
        return (lengths, plans) if want_plans else lengths

    def encode_device_ex_batch(self, members, want_plans: bool = False, want_device_plans: bool = False, stream: torch.cuda.Stream | None = None,
                               stats: dict | None = None):
        """Many block_ / carried-state mt_ streams in one call (hsrans_encode_device_ex_batch): member k is ``(container, states, bits,
        d_in, d_out)`` or ``(container, states, bits, d_in, d_out, options)`` with ``options`` a dict of ``encode_device_ex``'s keywords
        ``block_size``, ``independent_blocks``, ``index_interval``, ``index_groups`` and ``length`` (default ``d_in.numel()``).  Each
        member gets what ``encode_device_ex`` gives it.  Returns the stream lengths, followed by the list of plan blobs (``want_plans``)
        and/or the list of DevicePlans (``want_device_plans``), with None where a member asked for no index.  ``stats``: filled with
        hsrans_encode_ex_batch_stats.  Synchronous; the tensors are kept alive until it returns.  Raises HsransError naming the first
        failed member; the error carries ``code``, ``lengths``, ``rcs``, ``plans`` and ``device_plans`` (what the members that did not
        fail got)."""
        K = len(members)
        arr = (EncodeExMember * max(K, 1))()
        keep = []  # (tensors, options, group lists and plan buffers must outlive the call)
        blobs = [None] * K
        dev = None
        for k, m in enumerate(members):
            container, states, bits, d_in, d_out, o = _encode_member("encode_device_ex_batch", k, m,
                                                                     ("block_size", "independent_blocks", "index_interval", "index_groups", "length"))
            dev = d_in.device if dev is None else dev
            length = int(o.get("length", d_in.numel()))
            block_size, index_interval = int(o.get("block_size", 0)), int(o.get("index_interval", 0))
            groups = np.ascontiguousarray(o["index_groups"], dtype=np.uint64) if o.get("index_groups") is not None else None
            if groups is not None and groups.size == 0:  # a stream too short for more than one chain (as encode_device_ex)
                groups, index_interval = None, 4
            n_groups = 0 if groups is None else groups.size
            indexed = index_interval != 0 or n_groups != 0
            if indexed:
                pcap = (self.L.hsrans_plan_capacity_chains(container, states, length, n_groups, block_size) if n_groups
                        else self.L.hsrans_plan_capacity(container, states, length, index_interval, block_size))
                blobs[k] = np.zeros(max(pcap, 1), np.uint8)
            opts = EncodeOpts(block_size, 0 if n_groups else index_interval, blobs[k].ctypes.data if indexed else None, blobs[k].size if indexed else 0, 0,
                              ENC_INDEPENDENT_BLOCKS if o.get("independent_blocks") else 0, 0, groups.ctypes.data if n_groups else None, n_groups)
            keep += [d_in, d_out, groups, opts]
            e = arr[k]
            e.container, e.states, e.bits = container, states, bits
            e.d_in, e.length = d_in.data_ptr(), length
            e.d_out, e.out_capacity = d_out.data_ptr(), d_out.numel()
            e.opts = ctypes.pointer(opts)
        handles = (_vp * max(K, 1))()
        st = EncodeExBatchStats()
        rc = self.L.hsrans_encode_device_ex_batch(self.handle, arr, K, _stream(stream, dev), handles if want_device_plans else None, ctypes.byref(st))
        if stats is not None:
            stats.update(_as_dict(st))
        lengths = [int(arr[k].stream_length) for k in range(K)]
        plans = [blobs[k][: arr[k].opts.contents.plan_size].copy() if blobs[k] is not None and lengths[k] else None for k in range(K)]
        dplans = [DevicePlan(self, _vp(handles[k])) if want_device_plans and handles[k] else None for k in range(K)]
        del keep
        if rc != 0:
            rcs = [int(arr[k].rc) for k in range(K)]
            failed = [k for k in range(K) if rcs[k] != 0]
            raise _members_error("hsrans_encode_device_ex_batch", rc, failed if len(failed) < K else [], lengths=lengths, rcs=rcs, plans=plans, device_plans=dplans)
        out = [lengths]
        if want_plans:
            out.append(plans)
        if want_device_plans:
            out.append(dplans)
        return out[0] if len(out) == 1 else tuple(out)

    # -- multi-byte elements as byte planes ----------------------------------------------------------------------------
    @staticmethod
    def _plane_ptrs(d_planes, itemsize: int):
        d_planes = list(d_planes)
        if len(d_planes) != itemsize:
            raise HsransError(f"one plane per byte of an element: {itemsize} planes, not {len(d_planes)}")
        return _tensor_arrays(d_planes)[0]  # (an element has at least one byte: never an empty array)

    def planes_split_device(self, tensor: torch.Tensor, d_planes, elements: int | None = None, stream: torch.cuda.Stream | None = None):
        """hsrans_planes_split_device: the elements of a contiguous CUDA tensor (2-, 4- or 8-byte items) into ``d_planes`` (one uint8
        tensor of at least ``elements`` bytes per byte of an item).  Asynchronous on ``stream`` (default: torch's current stream)."""
        W = tensor.element_size()
        _check(self.L.hsrans_planes_split_device(self.handle, W, tensor.data_ptr(), tensor.numel() if elements is None else elements,
                                                 self._plane_ptrs(d_planes, W), _stream(stream, tensor.device)), "hsrans_planes_split_device")

    def planes_merge_device(self, d_planes, out_tensor: torch.Tensor, elements: int | None = None, stream: torch.cuda.Stream | None = None):
        """hsrans_planes_merge_device: ``d_planes`` interleaved back into the elements of ``out_tensor``.  Asynchronous on ``stream``."""
        W = out_tensor.element_size()
        _check(self.L.hsrans_planes_merge_device(self.handle, W, self._plane_ptrs(d_planes, W), out_tensor.numel() if elements is None else elements,
                                                 out_tensor.data_ptr(), _stream(stream, out_tensor.device)), "hsrans_planes_merge_device")

    def encode_device_planes(self, tensor: torch.Tensor, d_frame: torch.Tensor, d_work: torch.Tensor, states: int = 64, bits: int = 11,
                             block_size: int = 1 << 16, index_interval: int = 32, store_incompressible: bool = True, want_plans: bool = True,
                             stream: torch.cuda.Stream | None = None):
        """hsrans_encode_device_planes: a contiguous CUDA tensor whose ``element_size()`` is 2, 4 or 8, taken as bytes, into a frame of
        byte planes at ``d_frame`` (``planes_capacity`` bytes; ``d_work``: ``planes_workspace_bytes``).  Returns ``(frame_length, desc,
        plans)``: ``desc`` a PlanesDesc, ``plans`` a DevicePlan per plane (None for a stored plane; all None without ``want_plans``)."""
        return self._encode_planes("encode_device_planes", tensor, None, d_frame, d_work, states, bits, block_size, index_interval, store_incompressible, want_plans, stream)

    def _encode_planes(self, entry, tensor, based, d_frame, d_work, states, bits, block_size, index_interval, store_incompressible, want_plans, stream):
        """encode_device_planes (``based`` None) and encode_device_planes_delta / _diff (the base's pointer and bytes): one tensor into its frame"""
        if not tensor.is_contiguous():
            raise HsransError(f"{entry} takes a contiguous tensor")
        W = tensor.element_size()
        desc = PlanesDesc()
        handles = (_vp * PLANES_MAX)()
        head = (self.handle, W, states, bits, tensor.data_ptr())
        tail = (tensor.numel(), d_frame.data_ptr(), d_frame.numel(), block_size, index_interval, PLANES_STORE_INCOMPRESSIBLE if store_incompressible else 0,
                d_work.data_ptr(), d_work.numel(), _stream(stream, tensor.device), ctypes.byref(desc), handles if want_plans else None)
        n = self.L.hsrans_encode_device_planes(*head, *tail) if based is None else getattr(self.L, "hsrans_" + entry)(*head, *based, *tail)
        if n == 0:
            raise HsransError(f"hsrans_{entry} failed")
        plans = [DevicePlan(self, _vp(handles[p])) if want_plans and handles[p] else None for p in range(W)]
        return n, desc, plans

    def make_planes(self, desc: PlanesDesc, plans) -> Planes:
        """hsrans_planes_create: ``plans[p]`` is plane p's DevicePlan, None exactly for the stored planes."""
        plans = list(plans)
        if len(plans) != desc.elem_size:
            raise HsransError(f"one plan (or None) per plane: {desc.elem_size}, not {len(plans)}")
        h = _vp()
        _check(self.L.hsrans_planes_create(self.handle, ctypes.byref(desc), _handle_array(plans, PLANES_MAX), ctypes.byref(h)), "hsrans_planes_create")
        return Planes(self, h, desc, plans)

    def decode_device_planes(self, planes: Planes, d_frame: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                             stream: torch.cuda.Stream | None = None, frame_length: int | None = None):
        """hsrans_decode_device_planes: the frame at ``d_frame`` back into the elements of ``out_tensor`` (contiguous, as many bytes as
        were encoded).  Asynchronous on ``stream`` (default: torch's current stream)."""
        if not out_tensor.is_contiguous():
            raise HsransError("decode_device_planes takes a contiguous output tensor")
        _check(self.L.hsrans_decode_device_planes(self.handle, planes.handle, d_frame.data_ptr(), d_frame.numel() if frame_length is None else frame_length,
                                                  out_tensor.data_ptr(), out_tensor.numel() * out_tensor.element_size(), d_work.data_ptr(), d_work.numel(),
                                                  _stream(stream, d_frame.device)), "hsrans_decode_device_planes")

    def planes_status(self, planes: Planes, stream: torch.cuda.Stream | None = None) -> list:
        codes = (ctypes.c_int * PLANES_MAX)()
        self.L.hsrans_planes_status(self.handle, planes.handle, _stream(stream), codes)
        return list(codes)[: planes.desc.elem_size]

    def encode_device_planes_batch(self, tensors, d_frames, d_work: torch.Tensor, states: int = 64, bits: int = 11, block_size: int = 1 << 16,
                                   index_interval: int = 32, store_incompressible: bool = True, want_plans: bool = True, options=None,
                                   stream: torch.cuda.Stream | None = None, stats: dict | None = None) -> list:
        """hsrans_encode_device_planes_batch: many contiguous CUDA tensors (``element_size()`` 2, 4 or 8, any mix) into their frames
        ``d_frames[k]`` (``planes_capacity`` bytes each) in one call; ``d_work``: ``planes_batch_workspace_bytes`` bytes.  The keywords are
        every member's settings; ``options`` (a list with a dict or None per member) overrides ``states``, ``bits``, ``block_size``,
        ``index_interval`` and ``store_incompressible`` for single members.  Each member gets what ``encode_device_planes`` gives it.
        Returns a list of ``(frame_length, desc, plans)`` as that call's.  ``stats``: filled with hsrans_planes_batch_stats.  Synchronous.
        Raises HsransError naming the first member at fault; the error carries ``code`` and ``rcs``."""
        return self._encode_planes_batch("encode_device_planes_batch", tensors, None, d_frames, d_work, options, want_plans, stream, stats, states=states, bits=bits,
                                         block_size=block_size, index_interval=index_interval, store_incompressible=store_incompressible)

    def _encode_planes_batch(self, entry, tensors, bases, d_frames, d_work, options, want_plans, stream, stats, **defaults) -> list:
        """encode_device_planes_batch (``bases`` None) and encode_device_planes_delta_batch / _diff_batch: many tensors into their frames"""
        tensors, d_frames = list(tensors), list(d_frames)
        K = len(tensors)
        if len(d_frames) != K or (options is not None and len(options) != K) or (bases is not None and len(bases) != K):
            raise HsransError(f"{entry}: one frame (and one options entry) per tensor: {K} tensors" + ("" if bases is None else ", and one base or None"))
        if any(not t.is_contiguous() for t in tensors):
            raise HsransError(f"{entry} takes contiguous tensors")
        arr = (PlanesMember * max(K, 1))()
        for k, t in enumerate(tensors):
            o = dict(options[k]) if options is not None and options[k] is not None else {}
            unknown = set(o) - set(defaults)
            if unknown:
                raise HsransError(f"{entry}: member {k}: unknown options {sorted(unknown)}")
            o = dict(defaults, **o)
            e = arr[k]
            e.elem_size, e.states, e.bits, e.block_size, e.index_interval = t.element_size(), o["states"], o["bits"], o["block_size"], o["index_interval"]
            e.flags = PLANES_STORE_INCOMPRESSIBLE if o["store_incompressible"] else 0
            e.d_in, e.elements = t.data_ptr(), t.numel()
            e.d_frame, e.frame_capacity = d_frames[k].data_ptr(), d_frames[k].numel()
        handles = (_vp * (max(K, 1) * PLANES_MAX))()
        st = PlanesBatchStats()
        tail = (K, d_work.data_ptr(), d_work.numel(), _stream(stream, d_work.device), handles if want_plans else None, ctypes.byref(st))
        if bases is None:
            rc = self.L.hsrans_encode_device_planes_batch(self.handle, arr, *tail)
        else:
            based = [_base_of(entry, b, t, optional=True) for b, t in zip(bases, tensors)]
            rc = getattr(self.L, "hsrans_" + entry)(self.handle, arr, (_vp * max(K, 1))(*[p for p, _ in based]), (_sz * max(K, 1))(*[n for _, n in based]), *tail)
        if stats is not None:
            stats.update(_as_dict(st))
        if rc != 0:
            rcs = [int(arr[k].rc) for k in range(K)]
            failed = [k for k in range(K) if rcs[k] != 0]
            raise _members_error(f"hsrans_{entry}", rc, failed if len(failed) < K else [], rcs=rcs)
        return [(int(arr[k].frame_length), PlanesDesc.from_buffer_copy(arr[k].desc),
                 [DevicePlan(self, _vp(handles[k * PLANES_MAX + p])) if want_plans and handles[k * PLANES_MAX + p] else None for p in range(arr[k].elem_size)])
                for k in range(K)]

    def make_planes_set(self, descs, plans_lists) -> PlanesSet:
        """hsrans_planes_set_create: ``descs[k]`` and ``plans_lists[k]`` are member k's PlanesDesc and its planes' DevicePlans (None exactly
        for the stored planes), as ``make_planes`` takes them for one frame."""
        descs, plans_lists = list(descs), [list(p) for p in plans_lists]
        K = len(descs)
        if len(plans_lists) != K or any(len(p) != d.elem_size for d, p in zip(descs, plans_lists)):
            raise HsransError("make_planes_set: one list of plans per descriptor, one plan (or None) per plane")
        darr = (PlanesDesc * max(K, 1))(*descs)
        harr = (_vp * (max(K, 1) * PLANES_MAX))()
        for k, plans in enumerate(plans_lists):
            harr[k * PLANES_MAX: k * PLANES_MAX + len(plans)] = list(_handle_array(plans))
        h = _vp()
        _check(self.L.hsrans_planes_set_create(self.handle, darr, harr, K, ctypes.byref(h)), "hsrans_planes_set_create")
        return PlanesSet(self, h, descs, plans_lists)

    def decode_device_planes_batch(self, pset: PlanesSet, d_frames, out_tensors, d_work: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """hsrans_decode_device_planes_batch: the frames ``d_frames[k]`` back into the elements of ``out_tensors[k]`` (contiguous, as many
        bytes as were encoded); ``d_work``: ``pset.info()["work_bytes"]`` bytes.  Asynchronous on ``stream`` (default: torch's current stream)."""
        d_frames, out_tensors = list(d_frames), list(out_tensors)
        if len(d_frames) != len(pset.descs) or len(out_tensors) != len(pset.descs):
            raise HsransError(f"decode_device_planes_batch: one frame and one output per member: {len(pset.descs)}")
        if any(not t.is_contiguous() for t in out_tensors):
            raise HsransError("decode_device_planes_batch takes contiguous output tensors")
        frames, frame_lengths = _tensor_arrays(d_frames)
        outs, out_caps = _tensor_arrays(out_tensors, [t.numel() * t.element_size() for t in out_tensors])
        _check(self.L.hsrans_decode_device_planes_batch(self.handle, pset.handle, frames, frame_lengths, outs, out_caps, d_work.data_ptr(), d_work.numel(),
                                                        _stream(stream, d_work.device)), "hsrans_decode_device_planes_batch")

    def planes_set_status(self, pset: PlanesSet, stream: torch.cuda.Stream | None = None) -> list:
        """hsrans_planes_set_status: synchronises ``stream`` and returns every member's status (its first failing plane's, else 0)"""
        codes = (ctypes.c_int * max(len(pset.descs), 1))()
        self.L.hsrans_planes_set_status(self.handle, pset.handle, _stream(stream), codes)
        return list(codes)[: len(pset.descs)]

    # -- tensors coded against a base: a delta frame is the ordinary frame of tensor ^ base, and does not name its base ----------------
    def planes_split_delta_device(self, tensor: torch.Tensor, base: torch.Tensor, d_planes, elements: int | None = None, stream: torch.cuda.Stream | None = None):
        """hsrans_planes_split_delta_device: ``planes_split_device`` of ``tensor ^ base`` (``base``: a contiguous CUDA tensor of the
        tensor's element size and element count).  Asynchronous on ``stream``."""
        self._planes_split_against("planes_split_delta_device", tensor, base, d_planes, elements, stream)

    def _planes_split_against(self, entry, tensor, base, d_planes, elements, stream):
        """planes_split_delta_device and planes_split_diff_device"""
        W = tensor.element_size()
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, W, tensor.data_ptr(), _base_of(entry, base, tensor)[0], tensor.numel() if elements is None else elements,
                                                  self._plane_ptrs(d_planes, W), _stream(stream, tensor.device)), "hsrans_" + entry)

    def planes_merge_delta_device(self, d_planes, base: torch.Tensor, out_tensor: torch.Tensor, elements: int | None = None, stream: torch.cuda.Stream | None = None):
        """hsrans_planes_merge_delta_device: ``d_planes`` interleaved and XORed with ``base`` into ``out_tensor``, which may be ``base``
        itself (the delta applied in place).  Asynchronous on ``stream``."""
        self._planes_merge_against("planes_merge_delta_device", d_planes, base, out_tensor, elements, stream)

    def _planes_merge_against(self, entry, d_planes, base, out_tensor, elements, stream):
        """planes_merge_delta_device and planes_merge_diff_device"""
        W = out_tensor.element_size()
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, W, self._plane_ptrs(d_planes, W), _base_of(entry, base, out_tensor)[0],
                                                  out_tensor.numel() if elements is None else elements, out_tensor.data_ptr(), _stream(stream, out_tensor.device)),
               "hsrans_" + entry)

    def encode_device_planes_delta(self, tensor: torch.Tensor, base: torch.Tensor, d_frame: torch.Tensor, d_work: torch.Tensor, states: int = 64, bits: int = 11,
                                   block_size: int = 1 << 16, index_interval: int = 32, store_incompressible: bool = True, want_plans: bool = True,
                                   stream: torch.cuda.Stream | None = None):
        """hsrans_encode_device_planes_delta: ``encode_device_planes`` of ``tensor ^ base`` without the buffer that holds it — byte for
        byte the same frame, descriptor and plans.  The frame does not name its base: decode it with the same base
        (``decode_device_planes_delta``); ``decode_device_planes`` gives ``tensor ^ base``.  Returns ``(frame_length, desc, plans)``."""
        return self._encode_planes("encode_device_planes_delta", tensor, _base_of("encode_device_planes_delta", base, tensor), d_frame, d_work, states, bits, block_size,
                                   index_interval, store_incompressible, want_plans, stream)

    def decode_device_planes_delta(self, planes: Planes, d_frame: torch.Tensor, base: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                   stream: torch.cuda.Stream | None = None, frame_length: int | None = None):
        """hsrans_decode_device_planes_delta: the frame at ``d_frame``, XORed with ``base``, into ``out_tensor`` — which may be ``base``
        itself: the delta is then applied in place.  Launches and workspace as ``decode_device_planes``.  Asynchronous on ``stream``."""
        self._decode_planes_against("decode_device_planes_delta", planes, d_frame, base, out_tensor, d_work, stream, frame_length)

    def _decode_planes_against(self, entry, planes, d_frame, base, out_tensor, d_work, stream, frame_length):
        """decode_device_planes_delta and decode_device_planes_diff"""
        if not out_tensor.is_contiguous():
            raise HsransError(f"{entry} takes a contiguous output tensor")
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, planes.handle, d_frame.data_ptr(), d_frame.numel() if frame_length is None else frame_length,
                                                  *_base_of(entry, base, out_tensor), out_tensor.data_ptr(), out_tensor.numel() * out_tensor.element_size(),
                                                  d_work.data_ptr(), d_work.numel(), _stream(stream, d_frame.device)), "hsrans_" + entry)

    def encode_device_planes_delta_batch(self, tensors, bases, d_frames, d_work: torch.Tensor, states: int = 64, bits: int = 11, block_size: int = 1 << 16,
                                         index_interval: int = 32, store_incompressible: bool = True, want_plans: bool = True, options=None,
                                         stream: torch.cuda.Stream | None = None, stats: dict | None = None) -> list:
        """hsrans_encode_device_planes_delta_batch: ``encode_device_planes_batch`` with member k coded against ``bases[k]``, or as it is
        where ``bases[k]`` is None; one base may serve many members.  Each member gets what ``encode_device_planes_delta`` (None:
        ``encode_device_planes``) gives it.  Returns, fills ``stats`` and raises as that call."""
        return self._encode_planes_batch("encode_device_planes_delta_batch", tensors, list(bases), d_frames, d_work, options, want_plans, stream, stats, states=states,
                                         bits=bits, block_size=block_size, index_interval=index_interval, store_incompressible=store_incompressible)

    def decode_device_planes_delta_batch(self, pset: PlanesSet, d_frames, bases, out_tensors, d_work: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """hsrans_decode_device_planes_delta_batch: ``decode_device_planes_batch`` with member k XORed with ``bases[k]`` (None: as it
        is); ``out_tensors[k]`` may be ``bases[k]`` itself.  Asynchronous on ``stream`` (default: torch's current stream)."""
        self._decode_planes_batch_against("decode_device_planes_delta_batch", pset, d_frames, bases, out_tensors, d_work, stream)

    def _decode_planes_batch_against(self, entry, pset, d_frames, bases, out_tensors, d_work, stream):
        """decode_device_planes_delta_batch and decode_device_planes_diff_batch"""
        d_frames, bases, out_tensors = list(d_frames), list(bases), list(out_tensors)
        K = len(pset.descs)
        if len(d_frames) != K or len(out_tensors) != K or len(bases) != K:
            raise HsransError(f"{entry}: one frame, one base (or None) and one output per member: {K}")
        if any(not t.is_contiguous() for t in out_tensors):
            raise HsransError(f"{entry} takes contiguous output tensors")
        frames, frame_lengths = _tensor_arrays(d_frames)
        outs, out_caps = _tensor_arrays(out_tensors, [t.numel() * t.element_size() for t in out_tensors])
        based = [_base_of(entry, b, t, optional=True) for b, t in zip(bases, out_tensors)]
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, pset.handle, frames, frame_lengths, (_vp * K)(*[p for p, _ in based]), (_sz * K)(*[n for _, n in based]),
                                                  outs, out_caps, d_work.data_ptr(), d_work.numel(), _stream(stream, d_work.device)), "hsrans_" + entry)

    def decode_device_planes_gather_delta(self, pg: PlanesGather, ranges, base: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                          stream: torch.cuda.Stream | None = None):
        """hsrans_decode_device_planes_gather_delta: ``decode_device_planes_gather`` of a delta frame — element ``offset + i`` of the
        frame XORed with element ``offset + i`` of ``base``, the WHOLE base tensor (the frame's element size and element count), which may
        not share memory with ``out_tensor`` or ``d_work``.  Asynchronous on ``stream``; ``ranges`` is read before the call returns."""
        self._planes_gather_against("decode_device_planes_gather_delta", pg, ranges, base, out_tensor, d_work, stream)

    def _planes_gather_against(self, entry, pg, ranges, base, out_tensor, d_work, stream):
        """decode_device_planes_gather_delta and decode_device_planes_gather_diff"""
        desc = pg.planes.desc
        if not out_tensor.is_contiguous():
            raise HsransError(f"{entry} takes a contiguous output tensor")
        if out_tensor.element_size() != desc.elem_size:
            raise HsransError(f"{entry}: the frame's elements are {desc.elem_size} bytes, the output tensor's {out_tensor.element_size()}")
        if d_work.dtype != torch.uint8:
            raise HsransError(f"{entry} takes a uint8 workspace tensor")
        if not (isinstance(base, torch.Tensor) and base.is_cuda and base.is_contiguous() and base.element_size() == desc.elem_size and base.numel() == desc.elements):
            raise HsransError(f"{entry}: the base is a contiguous CUDA tensor of the frame's element size and element count", code=2)
        arr = _ranges_array(ranges)
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, pg.handle, _p(arr) if arr.size else None, arr.shape[0], base.data_ptr(), base.numel() * base.element_size(),
                                                  out_tensor.data_ptr(), out_tensor.numel() * out_tensor.element_size(), d_work.data_ptr(), d_work.numel(),
                                                  _stream(stream, out_tensor.device)), "hsrans_" + entry)

    # -- tensors coded against a base as a zigzag difference: a diff frame is the ordinary frame of z = zigzag(tensor - base), the items read
    # as little-endian unsigned integers; it names neither its base nor its rule, and a delta call makes garbage of it -------------------
    def planes_split_diff_device(self, tensor: torch.Tensor, base: torch.Tensor, d_planes, elements: int | None = None, stream: torch.cuda.Stream | None = None):
        """hsrans_planes_split_diff_device: ``planes_split_device`` of z, the zigzag of ``tensor - base`` (``base``: a contiguous CUDA
        tensor of the tensor's element size and element count).  Asynchronous on ``stream``."""
        self._planes_split_against("planes_split_diff_device", tensor, base, d_planes, elements, stream)

    def planes_merge_diff_device(self, d_planes, base: torch.Tensor, out_tensor: torch.Tensor, elements: int | None = None, stream: torch.cuda.Stream | None = None):
        """hsrans_planes_merge_diff_device: ``d_planes`` interleaved into z, the zigzag undone and the difference added to ``base`` into
        ``out_tensor``, which may be ``base`` itself (in place).  Asynchronous on ``stream``."""
        self._planes_merge_against("planes_merge_diff_device", d_planes, base, out_tensor, elements, stream)

    def encode_device_planes_diff(self, tensor: torch.Tensor, base: torch.Tensor, d_frame: torch.Tensor, d_work: torch.Tensor, states: int = 64, bits: int = 11,
                                  block_size: int = 1 << 16, index_interval: int = 32, store_incompressible: bool = True, want_plans: bool = True,
                                  stream: torch.cuda.Stream | None = None):
        """hsrans_encode_device_planes_diff: ``encode_device_planes`` of z, the zigzag of ``tensor - base``, without the buffer that holds
        it — byte for byte the same frame, descriptor and plans.  The frame names neither its base nor its rule: decode it with the same
        base by ``decode_device_planes_diff``; ``decode_device_planes`` gives z.  Returns ``(frame_length, desc, plans)``."""
        return self._encode_planes("encode_device_planes_diff", tensor, _base_of("encode_device_planes_diff", base, tensor), d_frame, d_work, states, bits, block_size,
                                   index_interval, store_incompressible, want_plans, stream)

    def decode_device_planes_diff(self, planes: Planes, d_frame: torch.Tensor, base: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                  stream: torch.cuda.Stream | None = None, frame_length: int | None = None):
        """hsrans_decode_device_planes_diff: ``base`` plus the difference the frame at ``d_frame`` holds, into ``out_tensor`` — which may
        be ``base`` itself (in place).  Launches and workspace as ``decode_device_planes``.  Asynchronous on ``stream``."""
        self._decode_planes_against("decode_device_planes_diff", planes, d_frame, base, out_tensor, d_work, stream, frame_length)

    def encode_device_planes_diff_batch(self, tensors, bases, d_frames, d_work: torch.Tensor, states: int = 64, bits: int = 11, block_size: int = 1 << 16,
                                        index_interval: int = 32, store_incompressible: bool = True, want_plans: bool = True, options=None,
                                        stream: torch.cuda.Stream | None = None, stats: dict | None = None) -> list:
        """hsrans_encode_device_planes_diff_batch: ``encode_device_planes_delta_batch`` under the diff rule — member k gets what
        ``encode_device_planes_diff`` gives it against ``bases[k]``, ``encode_device_planes`` where ``bases[k]`` is None.  A call is
        all-diff.  Returns, fills ``stats`` and raises as that call."""
        return self._encode_planes_batch("encode_device_planes_diff_batch", tensors, list(bases), d_frames, d_work, options, want_plans, stream, stats, states=states,
                                         bits=bits, block_size=block_size, index_interval=index_interval, store_incompressible=store_incompressible)

    def decode_device_planes_diff_batch(self, pset: PlanesSet, d_frames, bases, out_tensors, d_work: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """hsrans_decode_device_planes_diff_batch: ``decode_device_planes_batch`` with member k's difference added to ``bases[k]`` (None:
        as it is); ``out_tensors[k]`` may be ``bases[k]`` itself.  Asynchronous on ``stream`` (default: torch's current stream)."""
        self._decode_planes_batch_against("decode_device_planes_diff_batch", pset, d_frames, bases, out_tensors, d_work, stream)

    def decode_device_planes_gather_diff(self, pg: PlanesGather, ranges, base: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                         stream: torch.cuda.Stream | None = None):
        """hsrans_decode_device_planes_gather_diff: ``decode_device_planes_gather`` of a diff frame — element ``offset + i`` of ``base``,
        the WHOLE base tensor (the frame's element size and element count), plus the difference element ``offset + i`` of the frame
        holds; the base may not share memory with ``out_tensor`` or ``d_work``.  Asynchronous on ``stream``; ``ranges`` is read before
        the call returns."""
        self._planes_gather_against("decode_device_planes_gather_diff", pg, ranges, base, out_tensor, d_work, stream)

    def pack_device(self, srcs, lengths, arena: torch.Tensor, stream: torch.cuda.Stream | None = None) -> list:
        """hsrans_pack_device: the first ``lengths[k]`` bytes of the CUDA uint8 tensors ``srcs[k]`` (``lengths`` None: all of each) side by
        side into ``arena``, each at a multiple of 16 and completed with zeros up to the next, in one launch.  Returns the offsets
        (K + 1 entries, the last the bytes used: ``pack_layout``'s).  Asynchronous on ``stream`` (default: torch's current stream)."""
        srcs = list(srcs)
        _pack_buffers("pack_device", srcs + [arena])
        if lengths is not None and (len(lengths) != len(srcs) or any(not 0 <= int(n) <= t.numel() for n, t in zip(lengths, srcs))):
            raise HsransError("pack_device: one length per source, none beyond its tensor", code=2)
        ptrs, lens = _tensor_arrays(srcs, lengths) if srcs else ((_vp * 1)(), (_sz * 1)())
        _check(self.L.hsrans_pack_device(self.handle, ptrs, lens, len(srcs), arena.data_ptr(), arena.numel(), _stream(stream, arena.device)), "hsrans_pack_device")
        return pack_layout(list(lens)[: len(srcs)])[1]

    def planes_pack_device(self, descs, d_frames, arena: torch.Tensor, stream: torch.cuda.Stream | None = None) -> tuple:
        """hsrans_planes_pack_device: the planes of the frames ``d_frames[k]`` (CUDA uint8 tensors, described by ``descs[k]``) into
        ``arena`` in one launch.  Returns ``(descs, frames)``: the packed descriptors and ``frames[k]``, the arena's slice that is member
        k's frame — what make_planes_set's decode, decode_device_planes and the gather creators take in place of the unpacked frame, with
        the same plans.  ``planes_pack_layout(descs)[2]`` is the arena's exact size.  Asynchronous on ``stream``."""
        descs, d_frames = list(descs), list(d_frames)
        K = len(descs)
        if len(d_frames) != K:
            raise HsransError(f"planes_pack_device: one frame per descriptor: {K}")
        _pack_buffers("planes_pack_device", d_frames + [arena])
        src, out = (PlanesDesc * max(K, 1))(*descs), (PlanesDesc * max(K, 1))()
        bases = (ctypes.c_uint64 * (K + 1))()
        frames, frame_lengths = _tensor_arrays(d_frames) if K else ((_vp * 1)(), (_sz * 1)())
        _check(self.L.hsrans_planes_pack_device(self.handle, src, frames, frame_lengths, K, arena.data_ptr(), arena.numel(), _stream(stream, arena.device), out, bases),
               "hsrans_planes_pack_device")
        packed = [PlanesDesc.from_buffer_copy(d) for d in out][:K]
        return packed, [arena[bases[k]: bases[k] + packed[k].frame_length] for k in range(K)]

    def make_planes_gather(self, planes: Planes, d_frame: torch.Tensor, frame_length: int | None = None) -> PlanesGather:
        """hsrans_planes_gather_create: binds ``planes`` to the frame in the CUDA uint8 tensor ``d_frame`` (16-byte aligned) for
        decode_device_planes_gather.  The object keeps ``planes`` and the tensor alive.  Raises HsransError (``.code``: 2 a bad argument, 3 a
        plane's plan has no entry points)."""
        h = _vp()
        _check(self.L.hsrans_planes_gather_create(self.handle, planes.handle, d_frame.data_ptr(), d_frame.numel() if frame_length is None else frame_length,
                                                  ctypes.byref(h)), "hsrans_planes_gather_create")
        return PlanesGather(self, h, planes, d_frame)

    def decode_device_planes_gather(self, pg: PlanesGather, ranges, out_tensor: torch.Tensor, d_work: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """Element ranges of a frame that stays compressed on the GPU (hsrans_decode_device_planes_gather): for every row (offset, length,
        dst_offset) of ``ranges`` ((N, 3) uint64 or a sequence of such rows), all in elements, the elements [offset, offset + length) of the
        tensor land at element ``dst_offset`` of ``out_tensor`` (contiguous, the frame's element size); nothing else of it is written.
        ``d_work``: a CUDA uint8 tensor, 16-byte aligned, of planes_gather_workspace_bytes(itemsize, N, total elements) bytes.  Asynchronous on
        ``stream`` (default: torch's current stream); ``ranges`` is read before the call returns.  Raises HsransError (``.code``: 2 a bad
        range, destination or buffer; nothing was launched)."""
        if not out_tensor.is_contiguous():
            raise HsransError("decode_device_planes_gather takes a contiguous output tensor")
        if out_tensor.element_size() != pg.planes.desc.elem_size:
            raise HsransError(f"decode_device_planes_gather: the frame's elements are {pg.planes.desc.elem_size} bytes, the output tensor's {out_tensor.element_size()}")
        if d_work.dtype != torch.uint8:
            raise HsransError("decode_device_planes_gather takes a uint8 workspace tensor")
        arr = _ranges_array(ranges)
        _check(self.L.hsrans_decode_device_planes_gather(self.handle, pg.handle, _p(arr) if arr.size else None, arr.shape[0], out_tensor.data_ptr(),
                                                         out_tensor.numel() * out_tensor.element_size(), d_work.data_ptr(), d_work.numel(),
                                                         _stream(stream, out_tensor.device)), "hsrans_decode_device_planes_gather")

    def decode_device_planes_gather_indirect(self, pg: PlanesGather, d_ranges: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                             count: torch.Tensor | None = None, max_count: int | None = None, max_elements: int | None = None,
                                             workspace: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """decode_device_planes_gather for ranges that are on the GPU (hsrans_decode_device_planes_gather_indirect): ``d_ranges`` is a
        contiguous CUDA tensor (N, 3) of int64 / uint64 rows (offset, length, dst_offset), in elements; ``count`` a CUDA int32 / uint32 scalar
        tensor with the number of rows in use (None: ``max_count``, itself N when None).  Both are read when the launches run, not here:
        nothing is copied to the host, nothing is waited for, and the call can be captured into a graph.  ``max_elements``: the most elements
        the rows fetch in all — it fixes the regions of ``d_work`` (a CUDA uint8 tensor of planes_gather_workspace_bytes(itemsize, max_count,
        max_elements) bytes); None: what ``d_work`` can hold for that ``max_count``.  ``workspace``: a CUDA uint8 tensor of at least
        planes_gather_indirect_workspace_bytes(itemsize, max_count) bytes that no other call in flight uses; allocated here when None.
        Returns the workspace.  Raises HsransError (``.code``) for what the host can check; rows or a count only the device can refuse leave
        ``out_tensor`` and ``d_work`` untouched and are reported by ``planes_gather_refused(pg)`` (5)."""
        return self._planes_gather_indirect("decode_device_planes_gather_indirect", pg, d_ranges, (), out_tensor, d_work, count, max_count, max_elements, workspace, stream)

    def decode_device_planes_gather_indirect_delta(self, pg: PlanesGather, d_ranges: torch.Tensor, base: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                                   count: torch.Tensor | None = None, max_count: int | None = None, max_elements: int | None = None,
                                                   workspace: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """hsrans_decode_device_planes_gather_indirect_delta: ``decode_device_planes_gather_indirect`` of a delta frame — element
        ``offset + i`` of the frame XORed with element ``offset + i`` of ``base``, the WHOLE base tensor (the frame's element size and
        element count), which may not share memory with any other buffer of the call.  Everything else — arguments, workspaces, launches,
        what is returned, raised and reported — is ``decode_device_planes_gather_indirect``'s."""
        desc = pg.planes.desc
        if not (isinstance(base, torch.Tensor) and base.is_cuda and base.is_contiguous() and base.element_size() == desc.elem_size and base.numel() == desc.elements):
            raise HsransError("decode_device_planes_gather_indirect_delta: the base is a contiguous CUDA tensor of the frame's element size and element count", code=2)
        return self._planes_gather_indirect("decode_device_planes_gather_indirect_delta", pg, d_ranges, (base.data_ptr(), base.numel() * base.element_size()), out_tensor,
                                            d_work, count, max_count, max_elements, workspace, stream)

    def _planes_gather_indirect(self, entry: str, pg, d_ranges, based: tuple, out_tensor, d_work, count, max_count, max_elements, workspace, stream):
        """decode_device_planes_gather_indirect and its delta form: ``based`` is empty, or the base's (pointer, bytes)"""
        W = pg.planes.desc.elem_size
        if not out_tensor.is_contiguous():
            raise HsransError(f"{entry} takes a contiguous output tensor")
        if out_tensor.element_size() != W:
            raise HsransError(f"{entry}: the frame's elements are {W} bytes, the output tensor's {out_tensor.element_size()}")
        if d_work.dtype != torch.uint8:
            raise HsransError(f"{entry} takes a uint8 workspace tensor")
        max_count, workspace = _indirect_args(d_ranges, 3, count, max_count, workspace, lambda n: planes_gather_indirect_workspace_bytes(W, n), out_tensor.device,
                                              stream)
        if max_elements is None:
            max_elements = max(0, d_work.numel() // W // 256 * 256 - 30 * max_count)
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, pg.handle, d_ranges.data_ptr(), None if count is None else count.data_ptr(), max_count, max_elements, *based,
                                                   out_tensor.data_ptr(), out_tensor.numel() * W, d_work.data_ptr(), d_work.numel(), workspace.data_ptr(),
                                                   workspace.numel(), _stream(stream, out_tensor.device)), "hsrans_" + entry)
        return workspace

    def planes_gather_refused(self, pg: PlanesGather, stream: torch.cuda.Stream | None = None) -> int:
        """hsrans_planes_gather_refused: synchronises ``stream`` and returns 5 once where a decode_device_planes_gather_indirect on the object
        was refused on the device since the last look, else 0"""
        return int(self.L.hsrans_planes_gather_refused(self.handle, pg.handle, _stream(stream)))

    def planes_gather_status(self, pg: PlanesGather, stream: torch.cuda.Stream | None = None) -> list:
        """hsrans_planes_gather_status: synchronises ``stream`` and returns every plane's status (stored planes: 0)"""
        codes = (ctypes.c_int * PLANES_MAX)()
        self.L.hsrans_planes_gather_status(self.handle, pg.handle, _stream(stream), codes)
        return list(codes)[: pg.planes.desc.elem_size]

    def make_planes_gather_set(self, pset: PlanesSet, d_frames, frame_lengths=None) -> PlanesGatherSet:
        """hsrans_planes_gather_set_create: binds member k of ``pset`` to the frame in the CUDA uint8 tensor ``d_frames[k]`` (16-byte
        aligned) for decode_device_planes_gather_batch.  The object keeps ``pset`` and the tensors alive.  Raises HsransError (``.code``: 2 a
        bad argument, 3 a plane's plan has no entry points)."""
        d_frames = list(d_frames)
        if len(d_frames) != len(pset.descs) or (frame_lengths is not None and len(frame_lengths) != len(d_frames)):
            raise HsransError(f"make_planes_gather_set: one frame (and one length) per member: {len(pset.descs)}", code=2)
        frames, lengths = _tensor_arrays(d_frames, frame_lengths)
        h = _vp()
        _check(self.L.hsrans_planes_gather_set_create(self.handle, pset.handle, frames, lengths, ctypes.byref(h)), "hsrans_planes_gather_set_create")
        return PlanesGatherSet(self, h, pset, d_frames)

    def decode_device_planes_gather_batch(self, pgs: PlanesGatherSet, rows, out_tensor: torch.Tensor, d_work: torch.Tensor, stream: torch.cuda.Stream | None = None):
        """Element ranges of many frames that stay compressed on the GPU, in one call (hsrans_decode_device_planes_gather_batch): for every
        row (member, offset, length, dst_offset) of ``rows``, the last three in that member's elements, the elements [offset, offset +
        length) of member ``member`` land at byte ``dst_offset * itemsize(member)`` of ``out_tensor`` (contiguous, any dtype: all rows
        share it); nothing else of it is written.  ``d_work``: a CUDA uint8 tensor, 16-byte aligned, of
        planes_gather_batch_workspace_bytes(largest itemsize, N, total elements) bytes.  Asynchronous on ``stream`` (default: torch's current
        stream); ``rows`` is read before the call returns.  Raises HsransError (``.code``: 2 a bad row, destination or buffer; nothing was
        launched)."""
        self._planes_gather_batch("decode_device_planes_gather_batch", pgs, (), rows, out_tensor, d_work, stream)

    def make_planes_base_set(self, pgs: PlanesGatherSet, bases) -> PlanesBaseSet:
        """hsrans_planes_base_set_create: ``bases[k]`` is the base member k of ``pgs`` is decoded against by the delta forms of the batch
        gathers — a contiguous CUDA tensor of the member's element size and element count — or None for a member that goes as it is.  One
        tensor may serve many members.  The object keeps ``pgs`` and the tensors alive.  Raises HsransError (``.code``: 2 a bad argument,
        among them a base that shares memory with a member's frame)."""
        bases = list(bases)
        descs = pgs.pset.descs
        K = len(descs)
        if len(bases) != K:
            raise HsransError(f"make_planes_base_set: one base (or None) per member: {K}", code=2)
        for b, d in zip(bases, descs):
            if b is not None and not (isinstance(b, torch.Tensor) and b.is_cuda and b.is_contiguous() and b.element_size() == d.elem_size and b.numel() == d.elements):
                raise HsransError("make_planes_base_set: a base is a contiguous CUDA tensor of its member's element size and element count, or None", code=2)
        h = _vp()
        _check(self.L.hsrans_planes_base_set_create(self.handle, pgs.handle, (_vp * max(K, 1))(*[None if b is None else b.data_ptr() for b in bases]),
                                                    (_sz * max(K, 1))(*[0 if b is None else b.numel() * b.element_size() for b in bases]), ctypes.byref(h)),
               "hsrans_planes_base_set_create")
        return PlanesBaseSet(self, h, pgs, bases)

    @staticmethod
    def _base_set_args(entry: str, pgs: PlanesGatherSet, base_set) -> tuple:
        if not (isinstance(base_set, PlanesBaseSet) and base_set.pgs is pgs and base_set.handle):
            raise HsransError(f"{entry}: a base set made for this gather set (make_planes_base_set)", code=2)
        return (base_set.handle,)

    def decode_device_planes_gather_batch_delta(self, pgs: PlanesGatherSet, base_set: PlanesBaseSet, rows, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                                stream: torch.cuda.Stream | None = None):
        """hsrans_decode_device_planes_gather_batch_delta: ``decode_device_planes_gather_batch`` with every row of member k XORed with the
        same elements of ``base_set``'s base k (None there: the row as it is).  No base may share memory with ``out_tensor`` or ``d_work``.
        Everything else is ``decode_device_planes_gather_batch``'s."""
        self._planes_gather_batch("decode_device_planes_gather_batch_delta", pgs, self._base_set_args("decode_device_planes_gather_batch_delta", pgs, base_set), rows,
                                  out_tensor, d_work, stream)

    def _planes_gather_batch(self, entry: str, pgs, based: tuple, rows, out_tensor, d_work, stream):
        """decode_device_planes_gather_batch and its delta form: ``based`` is empty, or holds the base set's handle"""
        if not out_tensor.is_contiguous():
            raise HsransError(f"{entry} takes a contiguous output tensor")
        if d_work.dtype != torch.uint8:
            raise HsransError(f"{entry} takes a uint8 workspace tensor")
        arr = _member_ranges_array(rows)
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, pgs.handle, *based, _p(arr) if arr.size else None, arr.shape[0], out_tensor.data_ptr(),
                                                   out_tensor.numel() * out_tensor.element_size(), d_work.data_ptr(), d_work.numel(), _stream(stream, out_tensor.device)),
               "hsrans_" + entry)

    def decode_device_planes_gather_batch_indirect(self, pgs: PlanesGatherSet, d_rows: torch.Tensor, out_tensor: torch.Tensor, d_work: torch.Tensor,
                                                   count: torch.Tensor | None = None, max_count: int | None = None, workspace: torch.Tensor | None = None,
                                                   stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """decode_device_planes_gather_batch for rows that are on the GPU (hsrans_decode_device_planes_gather_batch_indirect): ``d_rows`` is a
        contiguous CUDA tensor (N, 4) of int64 / uint64 rows (offset, length, dst_offset, member) — the memory layout of
        decode_device_gather_batch_indirect's rows, the first three in that member's elements; ``count`` a CUDA int32 / uint32 scalar tensor
        with the number of rows in use (None: ``max_count``, itself N when None).  Both are read when the launches run, not here: nothing is
        copied to the host, nothing is waited for, and the call can be captured into a graph.  ``d_work``: a CUDA uint8 tensor, 16-byte
        aligned, its size the capacity (planes_gather_batch_workspace_bytes bounds what any rows need).  ``workspace``: a CUDA uint8 tensor
        of at least planes_gather_batch_indirect_workspace_bytes(the set's coded planes, its largest itemsize, max_count) bytes that no
        other call in flight uses; allocated here when None.  Returns the workspace.  Raises HsransError (``.code``) for what the host can
        check; rows or a count only the device can refuse leave ``out_tensor`` and ``d_work`` untouched and are reported by
        ``planes_gather_set_refused(pgs)`` (5)."""
        return self._planes_gather_batch_indirect("decode_device_planes_gather_batch_indirect", pgs, (), d_rows, out_tensor, d_work, count, max_count, workspace, stream)

    def decode_device_planes_gather_batch_indirect_delta(self, pgs: PlanesGatherSet, base_set: PlanesBaseSet, d_rows: torch.Tensor, out_tensor: torch.Tensor,
                                                         d_work: torch.Tensor, count: torch.Tensor | None = None, max_count: int | None = None,
                                                         workspace: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> torch.Tensor:
        """hsrans_decode_device_planes_gather_batch_indirect_delta: ``decode_device_planes_gather_batch_indirect`` with every row of
        member k XORed with the same elements of ``base_set``'s base k (None there: the row as it is).  No base may share memory with any
        other buffer of the call.  Everything else — arguments, workspaces, launches, capturability, what is returned, raised and reported
        — is ``decode_device_planes_gather_batch_indirect``'s."""
        return self._planes_gather_batch_indirect("decode_device_planes_gather_batch_indirect_delta", pgs,
                                                  self._base_set_args("decode_device_planes_gather_batch_indirect_delta", pgs, base_set), d_rows, out_tensor, d_work, count,
                                                  max_count, workspace, stream)

    def _planes_gather_batch_indirect(self, entry: str, pgs, based: tuple, d_rows, out_tensor, d_work, count, max_count, workspace, stream):
        """decode_device_planes_gather_batch_indirect and its delta form: ``based`` is empty, or holds the base set's handle"""
        if not out_tensor.is_contiguous():
            raise HsransError(f"{entry} takes a contiguous output tensor")
        if d_work.dtype != torch.uint8:
            raise HsransError(f"{entry} takes a uint8 workspace tensor")
        max_count, workspace = _indirect_args(d_rows, 4, count, max_count, workspace,
                                              lambda n: planes_gather_batch_indirect_workspace_bytes(pgs.coded, pgs.max_itemsize, n), out_tensor.device, stream)
        _check(getattr(self.L, "hsrans_" + entry)(self.handle, pgs.handle, *based, d_rows.data_ptr(), None if count is None else count.data_ptr(), max_count,
                                                   out_tensor.data_ptr(), out_tensor.numel() * out_tensor.element_size(), d_work.data_ptr(), d_work.numel(),
                                                   workspace.data_ptr(), workspace.numel(), _stream(stream, out_tensor.device)), "hsrans_" + entry)
        return workspace

    def planes_gather_set_refused(self, pgs: PlanesGatherSet, stream: torch.cuda.Stream | None = None) -> int:
        """hsrans_planes_gather_set_refused: synchronises ``stream`` and returns 5 once where a decode_device_planes_gather_batch_indirect on
        the object was refused on the device since the last look, else 0"""
        return int(self.L.hsrans_planes_gather_set_refused(self.handle, pgs.handle, _stream(stream)))

    def planes_gather_set_status(self, pgs: PlanesGatherSet, stream: torch.cuda.Stream | None = None) -> list:
        """hsrans_planes_gather_set_status: synchronises ``stream`` and returns every member's status (its first failing plane's, else 0)"""
        K = len(pgs.pset.descs)
        codes = (ctypes.c_int * max(K, 1))()
        self.L.hsrans_planes_gather_set_status(self.handle, pgs.handle, _stream(stream), codes)
        return list(codes)[:K]

    def block_choices_device(self, container: int, states: int, bits: int, d_in: torch.Tensor, block_size: int = 0,
                             stream: torch.cuda.Stream | None = None) -> np.ndarray:
        """The block choice hsrans_encode_device_ex makes (hsrans_block_choices_device): BLOCK_CHOICE records, as block_choices()."""
        s = _stream(stream, d_in.device)
        args = (self.handle, container, states, bits, d_in.data_ptr(), d_in.numel(), block_size)
        n = self.L.hsrans_block_choices_device(*args, None, 0, s)
        if n == 0:
            raise HsransError("hsrans_block_choices_device failed")
        out = np.zeros(n, BLOCK_CHOICE)
        self.L.hsrans_block_choices_device(*args, out.ctypes.data, n, s)
        return out

    def index_build_at(self, container: int, states: int, bits: int, stream, groups) -> np.ndarray:
        stream = _u8(stream)
        groups = np.ascontiguousarray(groups, dtype=np.uint64)
        out_len = int(stream[:8].view(np.uint64)[0])
        pcap = self.L.hsrans_plan_capacity_chains(container, states, out_len, groups.size, 0)
        plan = np.zeros(pcap, np.uint8)
        n = self.L.hsrans_index_build_at(self.handle, container, states, bits, _p(stream), stream.size, _p(groups), groups.size, _p(plan), pcap)
        if n == 0:
            raise HsransError("hsrans_index_build_at failed")
        return plan[:n].copy()

    def decode_host_pipelined(self, container: int, states: int, bits: int, stream: torch.Tensor, out: torch.Tensor, plan, n_slices: int = 0) -> int:
        """Host tensors (ideally pinned); returns the decoded length (0 = failure).  hsrans_decode_host_pipelined."""
        plan = _u8(plan)
        return self.L.hsrans_decode_host_pipelined(self.handle, container, states, bits, stream.data_ptr(), stream.numel(), out.data_ptr(), out.numel(),
                                                   _p(plan), plan.size, n_slices)

    def encode_host_pipelined(self, states: int, bits: int, host_in, host_out, block_size: int = 1 << 16, index_interval: int = 0,
                              n_slices: int = 0):
        """mt_ encode (independent fixed-size blocks) of host bytes into a host buffer on the GPU, the PCIe legs overlapped
        (hsrans_encode_host_pipelined; twin of :meth:`decode_host_pipelined`).  ``host_in`` / ``host_out``: torch CPU uint8 tensors
        (ideally pinned) or numpy arrays; ``host_out`` needs ``capacity(MT, states, len(host_in))`` bytes.  Returns ``(length, plan)``,
        ``plan`` a numpy array when ``index_interval`` is set, else None."""
        def addr(a):
            if isinstance(a, torch.Tensor):
                if a.is_cuda or a.dtype != torch.uint8 or not a.is_contiguous():
                    raise HsransError("encode_host_pipelined takes contiguous uint8 CPU tensors")
                return a.data_ptr(), a.numel()
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous):
                raise HsransError("encode_host_pipelined takes contiguous uint8 numpy arrays")
            return a.ctypes.data, a.size
        p_in, n_in = addr(host_in)
        p_out, n_out = addr(host_out)
        plan = np.zeros(max(self.L.hsrans_plan_capacity(MT, states, n_in, index_interval, block_size) if index_interval else 1, 1), np.uint8)
        opts = EncodeOpts(block_size, index_interval, plan.ctypes.data if index_interval else None, plan.size if index_interval else 0, 0,
                          ENC_INDEPENDENT_BLOCKS, 0, None, 0)
        n = self.L.hsrans_encode_host_pipelined(self.handle, MT, states, bits, p_in, n_in, p_out, n_out, ctypes.byref(opts), n_slices)
        if n == 0:
            raise HsransError("hsrans_encode_host_pipelined failed")
        return n, (plan[: opts.plan_size].copy() if index_interval else None)

    def index_build(self, container: int, states: int, bits: int, stream, index_interval: int) -> np.ndarray:
        stream = _u8(stream)
        out_len = int(stream[:8].view(np.uint64)[0])
        pcap = self.L.hsrans_plan_capacity(container, states, out_len, index_interval, 0)
        plan = np.zeros(pcap, np.uint8)
        n = self.L.hsrans_index_build(self.handle, container, states, bits, _p(stream), stream.size, index_interval, _p(plan), pcap)
        if n == 0:
            raise HsransError("hsrans_index_build failed")
        return plan[:n].copy()
