"""The C ABI of include/hsrans_hip.h as ctypes sees it: the structures, the constants, the signature of every function (SIGNATURES, kept in
step with the header by tests/test_binding_signatures.py) and the loading of the library.  api.py holds everything built on top."""
from __future__ import annotations

import ctypes
import os

RAW, BLOCK, MT = 0, 1, 2
ENC_INDEPENDENT_BLOCKS = 1
_HERE = os.path.dirname(os.path.abspath(__file__))
_sz, _vp, _i, _u32, _u64, _f64, _cp, _P = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double, ctypes.c_char_p, ctypes.POINTER


class HsransError(RuntimeError):
    """``code``: the HSRANS_E_* value the C call returned, None for an error that stems from no return code"""

    def __init__(self, message: str = "", code: int | None = None):
        super().__init__(message)
        self.code = code


class Hist(ctypes.Structure):
    """reference hist_t (src/hist.h:16-20)"""
    _fields_ = [("symbolCount", ctypes.c_uint16 * 256), ("cumul", ctypes.c_uint16 * 256)]


class EncodeOpts(ctypes.Structure):
    _fields_ = [("block_size", _u32), ("index_interval", _u32), ("plan_out", _vp), ("plan_capacity", _sz), ("plan_size", _sz), ("flags", _u32),
                ("reserved", _u32), ("index_groups", _vp), ("n_index_groups", _sz)]


class EncodeMember(ctypes.Structure):
    """hsrans_encode_member: one stream of hsrans_encode_device_batch"""
    _fields_ = [("container", _i), ("states", _i), ("bits", _u32), ("block_size", _u32), ("d_in", _vp), ("length", _sz), ("d_out", _vp),
                ("out_capacity", _sz), ("hist", _vp), ("index_interval", _u32), ("index_groups", _vp), ("n_index_groups", _sz), ("stream_length", _sz)]


class EncodeBatchStats(ctypes.Structure):
    _fields_ = [(n, _u32) for n in ("launches", "raw_members", "mt_members", "mt_blocks")]


class EncodeExMember(ctypes.Structure):
    """hsrans_encode_ex_member: one stream of hsrans_encode_device_ex_batch"""
    _fields_ = [("container", _i), ("states", _i), ("bits", _u32), ("d_in", _vp), ("length", _sz), ("d_out", _vp), ("out_capacity", _sz),
                ("opts", ctypes.POINTER(EncodeOpts)), ("stream_length", _sz), ("rc", _i)]


class EncodeExBatchStats(ctypes.Structure):
    _fields_ = ([(n, _u32) for n in ("launches", "block_members", "mt_members", "units", "blocks")] +
                [(n, ctypes.c_double) for n in ("summaries_us", "walk_us", "chain_us", "plans_us")])


class IndexingMember(ctypes.Structure):
    """hsrans_indexing_member: one stream of hsrans_decode_device_indexing_batch"""
    _fields_ = [("dplan", _vp), ("d_stream", _vp), ("stream_length", _sz), ("d_out", _vp), ("out_capacity", _sz), ("index_interval", _u32), ("rc", _i),
                ("indexed", _vp)]


class IndexingBatchStats(ctypes.Structure):
    _fields_ = [(n, _u32) for n in ("launches", "walk_members", "mt_members", "tasks")]


class Calibration(ctypes.Structure):
    _fields_ = [("class_weights", _u32 * 8), ("class_finish_us_last_iteration", ctypes.c_double * 8), ("last_wave_us_before", ctypes.c_double),
                ("last_wave_us_after", ctypes.c_double), ("class_spread_us_before", ctypes.c_double), ("class_spread_us_after", ctypes.c_double),
                ("iterations", _u32), ("reserved", _u32), ("bytes", ctypes.c_uint64)]


class LaunchInfo(ctypes.Structure):
    _fields_ = [(n, _u32) for n in ("grid", "block", "lds_bytes", "waves_per_block", "chains", "shared_table", "walk", "two_level", "table_mode", "chains_per_wave")] + \
               [("class_weights", _u32 * 8), ("dynamic_groups", _u32), ("spread", _u32)]


class PlanKind(ctypes.Structure):
    _fields_ = [(n, _u32) for n in ("container", "states", "bits", "flags")] + [("decoded_len", ctypes.c_uint64)] + \
               [(n, _u32) for n in ("n_chains", "n_pieces", "shared_hist", "interval")]


class LaunchFacts(ctypes.Structure):
    _fields_ = [(n, _u32) for n in ("persistent", "table_mode", "dual", "n_groups", "groups_lean", "spread_min_block", "tickets", "index_pass", "single_valid",
                                    "single_ring_entries", "calibrating", "parts", "n_parts", "dealt")]


class BatchInfo(ctypes.Structure):
    _fields_ = [(n, _u32) for n in ("members", "launches", "direct_members", "solo_members", "grouped_members", "groups", "grid", "block", "lds_bytes")] + \
               [("class_weights", _u32 * 8), ("imbalance", ctypes.c_double)]


class QueueStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("submitted", "flushes", "launches", "batches_made", "batches_reused", "retargeted")]


class Shard(ctypes.Structure):
    _fields_ = [("first_chain", _u32), ("chain_count", _u32), ("out_begin", ctypes.c_uint64), ("out_end", ctypes.c_uint64)]


class ShardedInfo(ctypes.Structure):
    _fields_ = [("world", _u32), ("rank", _u32), ("parts", _u32), ("root", ctypes.c_int32), ("window_begin", ctypes.c_uint64), ("window_end", ctypes.c_uint64),
                ("out_base", ctypes.c_uint64), ("out_length", ctypes.c_uint64), ("decoded_length", ctypes.c_uint64), ("stream_length", ctypes.c_uint64),
                ("one_launch", _u32), ("reserved", _u32)]


class Range(ctypes.Structure):  # hsrans_range
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64), ("dst_offset", ctypes.c_uint64)]


class GatherTask(ctypes.Structure):  # hsrans_gather_task
    _fields_ = [("begin", ctypes.c_uint64), ("end", ctypes.c_uint64), ("dst_delta", ctypes.c_int64)]


class MemberRange(ctypes.Structure):  # hsrans_member_range
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64), ("dst_offset", ctypes.c_uint64), ("member", _u32), ("reserved", _u32)]


class GatherMember(ctypes.Structure):  # hsrans_gather_member
    _fields_ = [("decoded_len", ctypes.c_uint64), ("n_chains", _u32), ("states", _u32), ("interval", _u32), ("kind", _u32)]


class GatherBatchTask(ctypes.Structure):  # hsrans_gather_batch_task
    _fields_ = [("begin", ctypes.c_uint64), ("end", ctypes.c_uint64), ("dst_delta", ctypes.c_int64), ("member", _u32), ("reserved", _u32)]


class GatherSetInfo(ctypes.Structure):  # hsrans_gather_set_info_t
    _fields_ = [("members", _u32), ("launches", _u32)] + \
               [(n, _u32 * 6) for n in ("kind_members", "kind_tasks", "kind_entries", "kind_grid", "kind_waves", "kind_lds_bytes")]


PLANES_MAX = 8
PLANES_STORE_INCOMPRESSIBLE = 1
PACK_CHUNK = 8192  # HSRANS_PACK_CHUNK
PACK_MAX_ITEMS = 65536 * PLANES_MAX


class PlanesDesc(ctypes.Structure):  # hsrans_planes_desc
    _fields_ = [(n, _u32) for n in ("elem_size", "states", "bits", "block_size", "index_interval", "stored_mask")] + \
               [("elements", ctypes.c_uint64), ("offset", ctypes.c_uint64 * PLANES_MAX), ("length", ctypes.c_uint64 * PLANES_MAX), ("frame_length", ctypes.c_uint64)]


class PlanesInfo(ctypes.Structure):  # hsrans_planes_info_t
    _fields_ = [(n, _u32) for n in ("coded", "stored", "launches")]


class PlanesMember(ctypes.Structure):
    """hsrans_planes_member: one tensor of hsrans_encode_device_planes_batch"""
    _fields_ = [("elem_size", _u32), ("states", _i), ("bits", _u32), ("block_size", _u32), ("index_interval", _u32), ("flags", _u32), ("d_in", _vp),
                ("elements", _sz), ("d_frame", _vp), ("frame_capacity", _sz), ("desc", PlanesDesc), ("frame_length", _sz), ("rc", _i)]


class PlanesBatchStats(ctypes.Structure):  # hsrans_planes_batch_stats
    _fields_ = [(n, _u32) for n in ("launches", "members", "planes", "stored")]


class PlanesSetInfo(ctypes.Structure):  # hsrans_planes_set_info_t
    _fields_ = [(n, _u32) for n in ("members", "coded", "stored", "launches", "merge_tasks", "reserved")] + [("work_bytes", _sz)]


class PlanesGatherInfo(ctypes.Structure):  # hsrans_planes_gather_info_t
    _fields_ = [(n, _u32) for n in ("coded", "stored", "rows", "merge_tasks", "launches")]


class PlanesGatherIndirectInfo(ctypes.Structure):  # hsrans_planes_gather_indirect_info_t
    _fields_ = [(n, _u32) for n in ("coded", "stored", "max_rows", "merge_grid", "launches", "set_launches")]


class PlanesGatherTask(ctypes.Structure):  # hsrans_planes_gather_task
    _fields_ = [("src", ctypes.c_uint64), ("work_pos", ctypes.c_uint64), ("dst_delta", ctypes.c_int64), ("lo", _u32), ("hi", _u32)]


class PlanesGatherSetInfo(ctypes.Structure):  # hsrans_planes_gather_set_info_t
    _fields_ = [(n, _u32) for n in ("members", "coded", "stored", "rows", "merge_tasks", "launches")]


class PlanesGatherSetIndirectInfo(ctypes.Structure):  # hsrans_planes_gather_set_indirect_info_t
    _fields_ = [(n, _u32) for n in ("members", "coded", "stored", "max_rows", "merge_grid", "launches", "set_launches")]


class PlanesGatherBatchTask(ctypes.Structure):  # hsrans_planes_gather_batch_task
    _fields_ = [("src", ctypes.c_uint64), ("work_pos", ctypes.c_uint64), ("plane_step", ctypes.c_uint64), ("dst_delta", ctypes.c_int64), ("lo", _u32), ("hi", _u32),
                ("member", _u32), ("reserved", _u32)]


COMM_ID_BYTES = 128
SHARD_DECODE_ONLY, SHARD_DECODE_AND_EXCHANGE, SHARD_EXCHANGE_ONLY = 0, 1, 2


def lib_path() -> str:
    # HSRANS_LIB: A/B a differently built libhsrans_hip.so in one process environment (kernel tuning only)
    if os.environ.get("HSRANS_LIB"):
        return os.environ["HSRANS_LIB"]
    if os.environ.get("HSRANS_DEBUG_STAMPS"):  # the per-wave stamps only exist in the diagnostic build (make -C csrc stamps)
        stamps = os.path.join(_HERE, "lib", "libhsrans_hip_stamps.so")
        if not os.path.exists(stamps):
            raise HsransError("HSRANS_DEBUG_STAMPS needs the diagnostic library: make -C hypersonic_rans_amd/csrc stamps")
        main = os.path.join(_HERE, "lib", "libhsrans_hip.so")
        # (`make` alone does not rebuild it: numbers from a diagnostic library older than the product one are numbers of old code)
        if os.path.exists(main) and os.path.getmtime(stamps) + 1 < os.path.getmtime(main):
            raise HsransError("libhsrans_hip_stamps.so is older than libhsrans_hip.so: make -C hypersonic_rans_amd/csrc all stamps")
        return stamps
    return os.path.join(_HERE, "lib", "libhsrans_hip.so")


# name -> (restype, argtypes) of every function of include/hsrans_hip.h, in the header's order.  Handles and buffers are c_void_p (an int, a
# c_void_p, a ctypes array or None will do); POINTER(...) where the callers pass byref() of that type.
SIGNATURES = {
    "hsrans_capacity": (_sz, [_i, _i, _sz]),
    "hsrans_make_hist": (None, [_P(Hist), _vp, _sz, _u32]),
    "hsrans_encode": (_sz, [_i, _i, _u32, _vp, _sz, _vp, _sz, _P(Hist)]),
    "hsrans_index_boundaries": (_sz, [_vp, _i, _u32, _sz, _vp, _sz]),
    "hsrans_encode_ex": (_sz, [_i, _i, _u32, _vp, _sz, _vp, _sz, _P(Hist), _P(EncodeOpts)]),
    "hsrans_plan_capacity": (_sz, [_i, _i, _sz, _u32, _u32]),
    "hsrans_plan_capacity_chains": (_sz, [_i, _i, _sz, _sz, _u32]),
    "hsrans_plan_build": (_sz, [_i, _i, _u32, _vp, _sz, _sz, _vp, _sz]),
    "hsrans_plan_chain_count": (_u32, [_vp, _sz]),
    "hsrans_plan_decoded_length": (_u64, [_vp, _sz]),
    "hsrans_plan_slice": (_sz, [_vp, _sz, _u32, _u32, _vp, _sz]),
    "hsrans_plan_chain_range": (_i, [_vp, _sz, _u32, _u32, _P(_u64), _P(_u64)]),
    "hsrans_plan_thin": (_sz, [_vp, _sz, _vp, _sz, _vp, _sz]),
    "hsrans_plan_stream_ranges": (_i, [_vp, _sz, _u32, _u32, _P(_u64)]),
    "hsrans_cpu_level": (_i, []),
    "hsrans_decode_cpu": (_sz, [_i, _u32, _i, _i, _u32, _vp, _sz, _vp, _sz, _vp, _sz]),
    "hsrans_index_build_host": (_sz, [_i, _u32, _i, _i, _u32, _vp, _sz, _vp, _sz, _vp, _sz]),
    "hsrans_ctx_create": (_i, [_i, _P(_vp)]),
    "hsrans_ctx_destroy": (None, [_vp]),
    "hsrans_ctx_device_name": (_cp, [_vp]),
    "hsrans_ctx_host_index_chains": (_u32, [_vp]),
    "hsrans_decode_host": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _vp, _sz, _vp, _sz]),
    "hsrans_dplan_create": (_i, [_vp, _vp, _sz, _P(_vp)]),
    "hsrans_dplan_destroy": (None, [_vp]),
    "hsrans_decode_device": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_decode_device_window": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp]),
    "hsrans_decode_device_ranges": (_i, [_vp, _vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp]),
    "hsrans_decode_device_gather": (_i, [_vp, _vp, _vp, _sz, _vp, _u32, _vp, _sz, _vp]),
    "hsrans_gather_segment": (_u64, [_u64, _u32, _u32, _u32]),
    "hsrans_gather_tasks": (_sz, [_u64, _u32, _u32, _u32, _vp, _u32, _vp, _sz]),
    "hsrans_gather_workspace_bytes": (_sz, [_u32]),
    "hsrans_decode_device_gather_indirect": (_i, [_vp, _vp, _vp, _sz, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_gather_set_create": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "hsrans_gather_set_destroy": (None, [_vp]),
    "hsrans_decode_device_gather_batch": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp]),
    "hsrans_gather_set_status": (_i, [_vp, _vp, _vp, _vp]),
    "hsrans_gather_set_info": (_i, [_vp, _vp]),
    "hsrans_gather_batch_workspace_bytes": (_sz, [_u32, _u32]),
    "hsrans_decode_device_gather_batch_indirect": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_gather_set_refused": (_i, [_vp, _vp, _vp]),
    "hsrans_gather_set_indirect_info": (_i, [_vp, _u32, _sz, _vp]),
    "hsrans_gather_batch_tasks": (_sz, [_vp, _u32, _vp, _u32, _u32, _u32, _vp, _sz]),
    "hsrans_dplan_create_from_device_stream": (_i, [_vp, _i, _i, _u32, _vp, _sz, _sz, _vp, _P(_vp)]),
    "hsrans_dplan_read_plan": (_sz, [_vp, _vp, _sz]),
    "hsrans_dplan_status": (_i, [_vp, _vp, _vp]),
    "hsrans_dplan_batch_create": (_i, [_vp, _vp, _u32, _P(_vp)]),
    "hsrans_dplan_batch_destroy": (None, [_vp]),
    "hsrans_decode_device_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hsrans_dplan_batch_status": (_i, [_vp, _vp, _vp, _vp]),
    "hsrans_dplan_batch_info": (_i, [_vp, _P(BatchInfo)]),
    "hsrans_index_boundaries_batch": (_sz, [_vp, _i, _u32, _vp, _u32, _u32, _vp, _sz]),
    "hsrans_batch_deal": (_f64, [_vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "hsrans_dplan_batch_read_finish": (_sz, [_vp, _vp, _sz]),
    "hsrans_queue_create": (_i, [_vp, _u32, _P(_vp)]),
    "hsrans_queue_destroy": (None, [_vp]),
    "hsrans_queue_submit": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_queue_flush": (_i, [_vp, _vp]),
    "hsrans_queue_pending": (_u32, [_vp]),
    "hsrans_queue_stats": (_i, [_vp, _P(QueueStats)]),
    "hsrans_comm_unique_id": (_i, [_vp]),
    "hsrans_comm_create": (_i, [_vp, _vp, _i, _i, _P(_vp)]),
    "hsrans_comm_destroy": (None, [_vp]),
    "hsrans_comm_rank": (_i, [_vp]),
    "hsrans_comm_world": (_i, [_vp]),
    "hsrans_comm_rccl_version": (_i, []),
    "hsrans_shard_layout": (_i, [_vp, _sz, _u32, _u32, _vp, _vp, _vp]),
    "hsrans_sharded_create": (_i, [_vp, _vp, _vp, _sz, _u32, _vp, _i, _P(_vp)]),
    "hsrans_sharded_create_rank": (_i, [_vp, _i, _i, _vp, _sz, _u32, _vp, _i, _P(_vp)]),
    "hsrans_sharded_destroy": (None, [_vp]),
    "hsrans_sharded_info": (_i, [_vp, _P(ShardedInfo), _vp, _sz]),
    "hsrans_sharded_part_plan": (_vp, [_vp, _u32]),
    "hsrans_sharded_whole_plan": (_vp, [_vp]),
    "hsrans_decode_sharded": (_i, [_vp, _vp, _vp, _i, _vp]),
    "hsrans_sharded_wait_part": (_i, [_vp, _u32, _vp]),
    "hsrans_sharded_status": (_i, [_vp, _vp]),
    "hsrans_decode_device_indexing": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _u32, _vp, _P(_vp)]),
    "hsrans_decode_device_indexing_batch": (_i, [_vp, _P(IndexingMember), _u32, _vp, _P(IndexingBatchStats)]),
    "hsrans_encode_device": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _vp, _sz, _u32, _u32, _vp, _P(_vp)]),
    "hsrans_encode_device_ex": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _vp, _sz, _P(Hist), _P(EncodeOpts), _vp, _P(_vp)]),
    "hsrans_block_choices": (_sz, [_i, _i, _u32, _vp, _sz, _u32, _vp, _sz]),
    "hsrans_block_choices_device": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _u32, _vp, _sz, _vp]),
    "hsrans_encode_device_raw": (_sz, [_vp, _i, _u32, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _sz, _vp, _sz, _P(_sz), _vp, _P(_vp)]),
    "hsrans_encode_device_batch": (_i, [_vp, _P(EncodeMember), _u32, _vp, _P(_vp), _P(EncodeBatchStats)]),
    "hsrans_encode_device_ex_batch": (_i, [_vp, _P(EncodeExMember), _u32, _vp, _P(_vp), _P(EncodeExBatchStats)]),
    "hsrans_planes_capacity": (_sz, [_u32, _i, _sz]),
    "hsrans_planes_workspace_bytes": (_sz, [_u32, _sz]),
    "hsrans_planes_split": (_i, [_u32, _vp, _sz, _vp]),
    "hsrans_planes_merge": (_i, [_u32, _vp, _sz, _vp]),
    "hsrans_planes_split_device": (_i, [_vp, _u32, _vp, _sz, _vp, _vp]),
    "hsrans_planes_merge_device": (_i, [_vp, _u32, _vp, _sz, _vp, _vp]),
    "hsrans_encode_device_planes": (_sz, [_vp, _u32, _i, _u32, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _vp, _sz, _vp, _P(PlanesDesc), _P(_vp)]),
    "hsrans_planes_create": (_i, [_vp, _P(PlanesDesc), _P(_vp), _P(_vp)]),
    "hsrans_planes_destroy": (None, [_vp]),
    "hsrans_decode_device_planes": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_status": (_i, [_vp, _vp, _vp, _vp]),
    "hsrans_planes_info": (_i, [_vp, _P(PlanesInfo)]),
    "hsrans_planes_batch_workspace_bytes": (_sz, [_vp, _vp, _u32]),
    "hsrans_planes_batch_tasks": (_sz, [_vp, _u32, _vp]),
    "hsrans_encode_device_planes_batch": (_i, [_vp, _P(PlanesMember), _u32, _vp, _sz, _vp, _P(_vp), _P(PlanesBatchStats)]),
    "hsrans_planes_set_create": (_i, [_vp, _P(PlanesDesc), _P(_vp), _u32, _P(_vp)]),
    "hsrans_planes_set_destroy": (None, [_vp]),
    "hsrans_planes_set_info": (_i, [_vp, _P(PlanesSetInfo)]),
    "hsrans_decode_device_planes_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "hsrans_planes_set_status": (_i, [_vp, _vp, _vp, _vp]),
    "hsrans_pack_layout": (_sz, [_vp, _u32, _vp]),
    "hsrans_pack_tasks": (_sz, [_vp, _u32, _vp]),
    "hsrans_pack_device": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp]),
    "hsrans_planes_pack_layout": (_sz, [_P(PlanesDesc), _u32, _P(PlanesDesc), _vp]),
    "hsrans_planes_pack_device": (_i, [_vp, _P(PlanesDesc), _vp, _vp, _u32, _vp, _sz, _vp, _P(PlanesDesc), _vp]),
    "hsrans_planes_gather_create": (_i, [_vp, _vp, _vp, _sz, _P(_vp)]),
    "hsrans_planes_gather_destroy": (None, [_vp]),
    "hsrans_planes_gather_workspace_bytes": (_sz, [_u32, _u32, _u64]),
    "hsrans_decode_device_planes_gather": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_gather_status": (_i, [_vp, _vp, _vp, _vp]),
    "hsrans_planes_gather_info": (_i, [_vp, _P(PlanesGatherInfo)]),
    "hsrans_planes_gather_tasks": (_sz, [_vp, _u32, _u64, _vp, _sz]),
    "hsrans_planes_gather_indirect_workspace_bytes": (_sz, [_u32, _u32]),
    "hsrans_decode_device_planes_gather_indirect": (_i, [_vp, _vp, _vp, _vp, _u32, _u64, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_gather_refused": (_i, [_vp, _vp, _vp]),
    "hsrans_planes_gather_indirect_info": (_i, [_vp, _u32, _u64, _sz, _P(PlanesGatherIndirectInfo)]),
    "hsrans_planes_gather_set_create": (_i, [_vp, _vp, _vp, _vp, _P(_vp)]),
    "hsrans_planes_gather_set_destroy": (None, [_vp]),
    "hsrans_planes_gather_batch_workspace_bytes": (_sz, [_u32, _u32, _u64]),
    "hsrans_decode_device_planes_gather_batch": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_gather_set_status": (_i, [_vp, _vp, _vp, _vp]),
    "hsrans_planes_gather_set_info": (_i, [_vp, _P(PlanesGatherSetInfo)]),
    "hsrans_planes_gather_batch_tasks": (_sz, [_vp, _u32, _vp, _vp, _u32, _vp, _sz]),
    "hsrans_planes_gather_batch_indirect_workspace_bytes": (_sz, [_u32, _u32, _u32]),
    "hsrans_decode_device_planes_gather_batch_indirect": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_gather_set_refused": (_i, [_vp, _vp, _vp]),
    "hsrans_planes_gather_set_indirect_info": (_i, [_vp, _u32, _sz, _sz, _P(PlanesGatherSetIndirectInfo)]),
    "hsrans_planes_split_delta": (_i, [_u32, _vp, _vp, _sz, _vp]),
    "hsrans_planes_merge_delta": (_i, [_u32, _vp, _vp, _sz, _vp]),
    "hsrans_planes_split_delta_device": (_i, [_vp, _u32, _vp, _vp, _sz, _vp, _vp]),
    "hsrans_planes_merge_delta_device": (_i, [_vp, _u32, _vp, _vp, _sz, _vp, _vp]),
    "hsrans_encode_device_planes_delta": (_sz, [_vp, _u32, _i, _u32, _vp, _vp, _sz, _sz, _vp, _sz, _u32, _u32, _u32, _vp, _sz, _vp, _P(PlanesDesc), _P(_vp)]),
    "hsrans_decode_device_planes_delta": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_encode_device_planes_delta_batch": (_i, [_vp, _P(PlanesMember), _vp, _vp, _u32, _vp, _sz, _vp, _P(_vp), _P(PlanesBatchStats)]),
    "hsrans_decode_device_planes_delta_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "hsrans_decode_device_planes_gather_delta": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_decode_device_planes_gather_indirect_delta": (_i, [_vp, _vp, _vp, _vp, _u32, _u64, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_base_set_create": (_i, [_vp, _vp, _vp, _vp, _P(_vp)]),
    "hsrans_planes_base_set_destroy": (None, [_vp]),
    "hsrans_decode_device_planes_gather_batch_delta": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_decode_device_planes_gather_batch_indirect_delta": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_planes_split_diff": (_i, [_u32, _vp, _vp, _sz, _vp]),
    "hsrans_planes_merge_diff": (_i, [_u32, _vp, _vp, _sz, _vp]),
    "hsrans_planes_split_diff_device": (_i, [_vp, _u32, _vp, _vp, _sz, _vp, _vp]),
    "hsrans_planes_merge_diff_device": (_i, [_vp, _u32, _vp, _vp, _sz, _vp, _vp]),
    "hsrans_encode_device_planes_diff": (_sz, [_vp, _u32, _i, _u32, _vp, _vp, _sz, _sz, _vp, _sz, _u32, _u32, _u32, _vp, _sz, _vp, _P(PlanesDesc), _P(_vp)]),
    "hsrans_decode_device_planes_diff": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_encode_device_planes_diff_batch": (_i, [_vp, _P(PlanesMember), _vp, _vp, _u32, _vp, _sz, _vp, _P(_vp), _P(PlanesBatchStats)]),
    "hsrans_decode_device_planes_diff_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "hsrans_decode_device_planes_gather_diff": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsrans_index_build": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _u32, _vp, _sz]),
    "hsrans_index_build_at": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _vp, _sz, _vp, _sz]),
    "hsrans_hpipe_create": (_i, [_vp, _vp, _sz, _u32, _P(_vp)]),
    "hsrans_hpipe_decode": (_sz, [_vp, _vp, _sz, _vp, _sz]),
    "hsrans_hpipe_destroy": (None, [_vp]),
    "hsrans_decode_host_pipelined": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _vp, _sz, _vp, _sz, _u32]),
    "hsrans_encode_host_pipelined": (_sz, [_vp, _i, _i, _u32, _vp, _sz, _vp, _sz, _P(EncodeOpts), _u32]),
    "hsrans_host_register": (_i, [_vp, _vp, _sz]),
    "hsrans_host_unregister": (_i, [_vp, _vp]),
    "hsrans_ctx_calibrate": (_i, [_vp, _u32, _u32, _P(Calibration)]),
    "hsrans_ctx_calibrate_runs": (_i, [_vp, _u32, _u32, _u32, _P(Calibration)]),
    "hsrans_dplan_launch_info": (_i, [_vp, _P(LaunchInfo)]),
    "hsrans_dealt_shares": (_i, [_vp, _u32, _vp, _u32, _u32, _u64, _vp, _vp]),
    "hsrans_launch_choice": (_i, [_vp, _P(PlanKind), _P(LaunchFacts), _P(LaunchInfo), _cp, _sz]),
    "hsrans_debug_read_stamps": (_sz, [_vp, _vp, _sz]),
    "hsrans_version": (_cp, []),
}

_LIB = None  # (HSRANS_LIB when it was loaded, the library)


def load_library() -> ctypes.CDLL:
    """Loads lib/libhsrans_hip.so and declares every function of SIGNATURES on it; a name the library does not export raises AttributeError.
    Fails loudly when it has not been built (python -c 'import __graft_entry__ as g; g.build()').  Loaded once; again only when HSRANS_LIB
    names another file by then (tools/ab_probe.py runs several builds in one process)."""
    global _LIB
    asked = os.environ.get("HSRANS_LIB")
    if _LIB is not None and _LIB[0] == asked:
        return _LIB[1]
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` (there is no fallback implementation)")
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = (asked, L)
    return L
