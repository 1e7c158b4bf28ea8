"""ctypes binding of include/uvaia_gpu.h (the only way Python reaches the engine)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "lib", "libuvaia_gpu.so")
NSCORE = 6

# every symbol include/uvaia_gpu.h declares (tests check the library exports all of them)
SYMBOLS = [
    "uvaia_gpu_open", "uvaia_gpu_open_tuned", "uvaia_gpu_close", "uvaia_gpu_last_error", "uvaia_gpu_push", "uvaia_gpu_drain",
    "uvaia_gpu_heap_slots", "uvaia_gpu_n_query", "uvaia_gpu_reset", "uvaia_gpu_db_reserve", "uvaia_gpu_db_append",
    "uvaia_gpu_db_append_block", "uvaia_gpu_db_size", "uvaia_gpu_search_resident", "uvaia_gpu_sync", "uvaia_gpu_ball", "uvaia_gpu_ball_resident", "uvaia_gpu_ball_packed", "uvaia_gpu_unpack_rows", "uvaia_gpu_ball_asked", "uvaia_gpu_ball_kernel_ms", "uvaia_gpu_export_query_table", "uvaia_gpu_agree_on_polymorphic", "uvaia_gpu_query_columns",
    "uvaia_gpu_last_batch_scores", "uvaia_gpu_scan_stats", "uvaia_gpu_replay_stats", "uvaia_gpu_replay_tiles_opened", "uvaia_gpu_replay_timing",
    "uvaia_gpu_state_bytes", "uvaia_gpu_state_export", "uvaia_gpu_state_import", "uvaia_gpu_slice_scan", "uvaia_gpu_slice_replay",
    "uvaia_gpu_entered_flags", "uvaia_gpu_state_range_bytes", "uvaia_gpu_state_export_range", "uvaia_gpu_state_import_range",
    "uvaia_gpu_slice_replay_range", "uvaia_gpu_slice_buffers", "uvaia_gpu_scan_bytes_per_ref", "uvaia_gpu_derived_bytes_per_ref", "uvaia_gpu_scan_variant", "uvaia_gpu_set_query_tile", "uvaia_gpu_packed_bytes_per_ref",
    "uvaia_gpu_db_tile_bytes", "uvaia_gpu_db_side_row_ints", "uvaia_gpu_db_export", "uvaia_gpu_db_append_packed", "uvaia_gpu_db_clear", "uvaia_gpu_db_rederive", "uvaia_gpu_db_derived_export",
    "uvaia_gpu_set_active_queries", "uvaia_gpu_max_tolerance", "uvaia_gpu_search_resident_pool",
    "uvaia_gpu_db_set_shard", "uvaia_gpu_shard_rows", "uvaia_gpu_shard_scan", "uvaia_gpu_scan_wait", "uvaia_gpu_replay_wait", "uvaia_gpu_set_snapshot", "uvaia_gpu_shard_replay",
    "uvaia_gpu_mark", "uvaia_gpu_stream_wait_mark", "uvaia_gpu_wait_stream",
    "uvaia_gpu_shard_aux_bytes", "uvaia_gpu_db_skip", "uvaia_gpu_shard_set_peer", "uvaia_gpu_shard_planes", "uvaia_gpu_shard_side_rows",
    "uvaia_gpu_shard_ipc_handle_bytes", "uvaia_gpu_shard_ipc_handles", "uvaia_gpu_shard_ipc_open", "uvaia_gpu_shard_ipc_close",
    "uvaia_gpu_group_open", "uvaia_gpu_group_close", "uvaia_gpu_group_last_error", "uvaia_gpu_group_size", "uvaia_gpu_group_member", "uvaia_gpu_group_query_shard",
    "uvaia_gpu_group_db_reserve", "uvaia_gpu_group_db_append", "uvaia_gpu_group_db_append_packed", "uvaia_gpu_group_db_clear", "uvaia_gpu_group_db_rederive",
    "uvaia_gpu_group_db_size", "uvaia_gpu_group_reset", "uvaia_gpu_group_search_resident", "uvaia_gpu_group_push", "uvaia_gpu_group_drain", "uvaia_gpu_group_sync",
    "uvaia_gpu_rows_census", "uvaia_gpu_db_append_device", "uvaia_gpu_rows_exceptions", "uvaia_gpu_db_drop_tiles", "uvaia_gpu_rows_kernel_ms", "uvaia_gpu_rows_set_run_cut",
    "uvaia_gpu_db_stage_reserve", "uvaia_gpu_db_stage_packed", "uvaia_gpu_db_load_staged", "uvaia_gpu_db_unpack_rows", "uvaia_gpu_window_ms", "uvaia_gpu_free_bytes",
    "uvaia_gpu_db_stage_packed_at", "uvaia_gpu_db_append_staged", "uvaia_gpu_db_stage_compact_at", "uvaia_gpu_compact_ms",
    "uvaia_gpu_db_encode_compact", "uvaia_gpu_db_encoded_records", "uvaia_gpu_encode_ms",
    "uvaia_gpu_db_stage_unpack_rows", "uvaia_gpu_stage_unpack_ms",
    "uvaia_gpu_search_plan",
    "uvaia_gpu_fasta_open", "uvaia_gpu_fasta_close", "uvaia_gpu_fasta_last_error", "uvaia_gpu_fasta_scan", "uvaia_gpu_fasta_bad", "uvaia_gpu_fasta_records", "uvaia_gpu_fasta_rows", "uvaia_gpu_fasta_rows_host",
    "uvaia_gpu_fasta_kernel_ms", "uvaia_gpu_fasta_chunk_bytes", "uvaia_gpu_fasta_pinned_alloc", "uvaia_gpu_fasta_pinned_free",
    "uvaia_gpu_fasta_acgt", "uvaia_gpu_fasta_sequences", "uvaia_gpu_fasta_sequences_host", "uvaia_gpu_fasta_sequences_ms",
    "uvaia_gpu_text_append_device", "uvaia_gpu_text_size", "uvaia_gpu_text_rows", "uvaia_gpu_text_clear", "uvaia_gpu_text_reserve", "uvaia_gpu_text_ms",
    "uvaia_gpu_db_pairs", "uvaia_gpu_db_pairs_within", "uvaia_gpu_pairs_ms",
    "uvaia_gpu_db_link_begin", "uvaia_gpu_db_link", "uvaia_gpu_db_link_labels", "uvaia_gpu_link_ms",
    "uvaia_gpu_db_near_begin", "uvaia_gpu_db_near_components", "uvaia_gpu_db_near", "uvaia_gpu_db_near_fetch", "uvaia_gpu_db_mst", "uvaia_gpu_near_ms", "uvaia_gpu_near_tiles",
]

PAIR_NCOUNT = 5
PAIRS_SNP, PAIRS_COUNTS, PAIRS_SNP_ALT = 1, 2, 3        # `what` of uvaia_gpu_db_pairs
DIST_SNP, DIST_UVAIA = 1, 2                             # `metric` of uvaia_gpu_db_pairs_within
# uvaia_gpu_pair: (row, col, count[5])
PAIR_DTYPE = np.dtype([("row", np.uint32), ("col", np.uint32), ("count", np.int32, (PAIR_NCOUNT,))])
# uvaia_gpu_edge: (a, b, dist), a < b
EDGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("dist", np.int32)])
NEAR_NONE = 2 ** 64 - 1                                 # UVAIA_GPU_NEAR_NONE: no reference of another component is an edge away


class GpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("uvaia_gpu error %d: %s" % (code, msg))
        self.code = code


class Tuning(C.Structure):
    """uvaia_gpu_tuning: optional knobs of uvaia_gpu_open_tuned (0 = the library's choice); they change speed, never results."""
    _fields_ = [("subslice_refs", C.c_size_t), ("rare_max", C.c_int), ("scan", C.c_int), ("serial", C.c_int),
                ("scan_tiles_per_wave", C.c_int), ("scan_waves_per_block", C.c_int), ("rederive_streams", C.c_int), ("ball_gather", C.c_int), ("query_tables", C.c_int), ("replay_extras", C.c_int), ("replay_cus", C.c_int), ("scan_streams", C.c_int), ("pipeline", C.c_int), ("head_scan", C.c_int), ("derive_waves", C.c_int)]

    SCAN = {"auto": 0, "packed": 1, "compressed": 2, "wide": 3}

    @classmethod
    def make(cls, tuning):
        """None, a Tuning, or a dict such as {"scan": "compressed", "subslice_refs": 448, "serial": 1}"""
        if tuning is None or isinstance(tuning, cls):
            return tuning
        t = cls()
        for k, v in tuning.items():
            setattr(t, k, cls.SCAN[v] if k == "scan" and isinstance(v, str) else int(v))
        return t


class _Query(C.Structure):
    _fields_ = [
        ("n_query", C.c_int), ("nchar", C.c_int),
        ("seq", C.POINTER(C.c_char_p)), ("consensus", C.c_char_p),
        ("idx_c", C.POINTER(C.c_size_t)), ("idx_m", C.POINTER(C.c_size_t)), ("idx", C.POINTER(C.c_size_t)),
        ("n_idx_c", C.c_int), ("n_idx_m", C.c_int), ("n_idx", C.c_int),
        ("trim", C.c_size_t), ("acgt", C.c_int),
    ]


def library_path():
    return _LIB


def build_library(force=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".inc"))] + [os.path.join(ROOT, "include", "uvaia_gpu.h")]
    if not force and os.path.exists(_LIB) and os.path.getmtime(_LIB) >= max(os.path.getmtime(f) for f in srcs):
        return _LIB
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s"])
    return _LIB


_lib = None


def load_library():
    """Load libuvaia_gpu.so; raises if it has not been built (there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise GpuError(-2, "HIP library %s is missing: run __graft_entry__.build() (no CPU fallback exists)" % _LIB)
    L = C.CDLL(_LIB)
    vp = C.c_void_p
    pp = C.POINTER(C.c_char_p)
    pi = C.POINTER(C.c_int)
    sig = {
        "uvaia_gpu_open": (C.c_int, [C.POINTER(vp), C.POINTER(_Query), C.c_int, C.c_int, C.c_size_t]),
        "uvaia_gpu_open_tuned": (C.c_int, [C.POINTER(vp), C.POINTER(_Query), C.c_int, C.c_int, C.c_size_t, C.POINTER(Tuning)]),
        "uvaia_gpu_close": (None, [vp]),
        "uvaia_gpu_last_error": (C.c_char_p, [vp]),
        "uvaia_gpu_push": (C.c_int, [vp, pp, pi, C.c_int, C.c_int64, C.POINTER(C.c_uint8)]),
        "uvaia_gpu_drain": (C.c_int, [vp, pi, pi, pi, C.POINTER(C.c_int64)]),
        "uvaia_gpu_heap_slots": (C.c_int, [vp]),
        "uvaia_gpu_n_query": (C.c_int, [vp]),
        "uvaia_gpu_reset": (C.c_int, [vp]),
        "uvaia_gpu_db_reserve": (C.c_int, [vp, C.c_size_t]),
        "uvaia_gpu_db_append": (C.c_int, [vp, pp, pi, C.c_int]),
        "uvaia_gpu_db_append_block": (C.c_int, [vp, C.c_void_p, C.c_size_t, pi, C.c_int]),
        "uvaia_gpu_db_size": (C.c_size_t, [vp]),
        "uvaia_gpu_search_resident": (C.c_int, [vp, C.c_size_t, C.c_int64, C.POINTER(C.c_uint8)]),
        "uvaia_gpu_sync": (C.c_int, [vp]),
        "uvaia_gpu_ball": (C.c_int, [vp, pp, C.c_int, C.c_int, pi]),
        "uvaia_gpu_ball_resident": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_int, pi]),
        "uvaia_gpu_ball_packed": (C.c_int, [vp, C.c_void_p, C.c_int, C.c_int, pi]),
        "uvaia_gpu_unpack_rows": (C.c_int, [vp, pi, C.c_int, C.c_void_p, C.c_size_t]),
        "uvaia_gpu_ball_asked": (C.c_ulonglong, [vp, C.c_int]),
        "uvaia_gpu_ball_kernel_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_export_query_table": (C.c_int, [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "uvaia_gpu_agree_on_polymorphic": (C.c_int, [vp, pp, C.c_int, C.POINTER(C.c_uint8)]),
        "uvaia_gpu_query_columns": (C.c_int, [pp, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_uint8)]),
        "uvaia_gpu_last_batch_scores": (C.c_int, [vp, pi, C.c_int]),
        "uvaia_gpu_scan_stats": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_replay_stats": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.c_int]),
        "uvaia_gpu_replay_tiles_opened": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.c_int]),
        "uvaia_gpu_replay_timing": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.c_int]),
        "uvaia_gpu_state_bytes": (C.c_size_t, [vp]),
        "uvaia_gpu_state_export": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_state_import": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_slice_scan": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_int]),
        "uvaia_gpu_slice_replay": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int]),
        "uvaia_gpu_entered_flags": (C.c_int, [vp, C.POINTER(C.c_uint8), C.c_int]),
        "uvaia_gpu_state_range_bytes": (C.c_size_t, [vp, C.c_int, C.c_int]),
        "uvaia_gpu_state_export_range": (C.c_int, [vp, C.c_void_p, C.c_int, C.c_int]),
        "uvaia_gpu_state_import_range": (C.c_int, [vp, C.c_void_p, C.c_int, C.c_int]),
        "uvaia_gpu_slice_replay_range": (C.c_int, [vp, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int]),
        "uvaia_gpu_slice_buffers": (C.c_int, []),
        "uvaia_gpu_scan_bytes_per_ref": (C.c_size_t, [vp]),
        "uvaia_gpu_derived_bytes_per_ref": (C.c_size_t, [vp]),
        "uvaia_gpu_scan_variant": (C.c_int, [vp]),
        "uvaia_gpu_set_query_tile": (C.c_int, [vp, C.c_int]),
        "uvaia_gpu_packed_bytes_per_ref": (C.c_size_t, [vp]),
        "uvaia_gpu_set_active_queries": (C.c_int, [vp, C.c_int, C.c_int]),
        "uvaia_gpu_max_tolerance": (C.c_int, [vp, pi]),
        "uvaia_gpu_search_resident_pool": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_int64, C.c_int]),
        "uvaia_gpu_db_tile_bytes": (C.c_size_t, [vp]),
        "uvaia_gpu_db_clear": (C.c_int, [vp]),
        "uvaia_gpu_db_rederive": (C.c_int, [vp]),
        "uvaia_gpu_db_derived_export": (C.c_int, [vp, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "uvaia_gpu_db_side_row_ints": (C.c_int, []),
        "uvaia_gpu_db_export": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_void_p, pi, pi]),
        "uvaia_gpu_db_append_packed": (C.c_int, [vp, C.c_void_p, pi, pi, C.c_int]),
        "uvaia_gpu_db_set_shard": (C.c_int, [vp, C.c_int, C.c_int, C.c_size_t]),
        "uvaia_gpu_shard_rows": (C.c_int, [vp]),
        "uvaia_gpu_shard_scan": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
        "uvaia_gpu_shard_aux_bytes": (C.c_size_t, [vp, C.c_size_t]), "uvaia_gpu_db_skip": (C.c_int, [vp, C.c_size_t]),
        "uvaia_gpu_shard_set_peer": (C.c_int, [vp, C.c_int, C.c_void_p, C.c_void_p]),
        "uvaia_gpu_shard_planes": (C.c_void_p, [vp]), "uvaia_gpu_shard_side_rows": (C.c_void_p, [vp]),
        "uvaia_gpu_shard_ipc_handle_bytes": (C.c_int, []), "uvaia_gpu_shard_ipc_handles": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_shard_ipc_open": (C.c_int, [vp, C.c_int, C.c_void_p]), "uvaia_gpu_shard_ipc_close": (C.c_int, [vp]),
        "uvaia_gpu_scan_wait": (C.c_int, [vp]),
        "uvaia_gpu_replay_wait": (C.c_int, [vp]),
        "uvaia_gpu_set_snapshot": (C.c_int, [vp, C.c_int]),
        "uvaia_gpu_shard_replay": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int64, C.c_int, C.c_int]),
        "uvaia_gpu_mark": (C.c_int, [vp, C.c_int, C.c_int]), "uvaia_gpu_stream_wait_mark": (C.c_int, [vp, C.c_void_p, C.c_int]),
        "uvaia_gpu_wait_stream": (C.c_int, [vp, C.c_int, C.c_void_p]),
        "uvaia_gpu_group_open": (C.c_int, [C.POINTER(vp), C.POINTER(_Query), C.c_int, pi, C.c_int, C.c_size_t, C.c_size_t]),
        "uvaia_gpu_group_close": (None, [vp]),
        "uvaia_gpu_group_last_error": (C.c_char_p, [vp]),
        "uvaia_gpu_group_size": (C.c_int, [vp]),
        "uvaia_gpu_group_member": (vp, [vp, C.c_int]),
        "uvaia_gpu_group_query_shard": (C.c_int, [vp, C.c_int, pi, pi]),
        "uvaia_gpu_group_db_reserve": (C.c_int, [vp, C.c_size_t]),
        "uvaia_gpu_group_db_append": (C.c_int, [vp, pp, pi, C.c_int]),
        "uvaia_gpu_group_db_append_packed": (C.c_int, [vp, C.c_void_p, pi, pi, C.c_int]),
        "uvaia_gpu_group_db_clear": (C.c_int, [vp]),
        "uvaia_gpu_group_db_rederive": (C.c_int, [vp]),
        "uvaia_gpu_group_db_size": (C.c_size_t, [vp]),
        "uvaia_gpu_group_reset": (C.c_int, [vp]),
        "uvaia_gpu_group_search_resident": (C.c_int, [vp, C.c_size_t, C.c_int64, C.POINTER(C.c_uint8)]),
        "uvaia_gpu_group_push": (C.c_int, [vp, pp, pi, C.c_int, C.c_int64, C.POINTER(C.c_uint8)]),
        "uvaia_gpu_group_drain": (C.c_int, [vp, pi, pi, pi, C.POINTER(C.c_int64)]),
        "uvaia_gpu_group_sync": (C.c_int, [vp]),
        "uvaia_gpu_rows_census": (C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_int, pi, pi]),
        "uvaia_gpu_db_append_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, pi, C.c_int, pi]),
        "uvaia_gpu_rows_exceptions": (C.c_int, [vp, C.c_void_p, C.c_size_t, pi, C.c_int, C.POINTER(C.c_uint64), C.c_void_p]),
        "uvaia_gpu_db_drop_tiles": (C.c_int, [vp, C.c_size_t]),
        "uvaia_gpu_rows_kernel_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_rows_set_run_cut": (C.c_int, [vp, C.c_uint]),
        "uvaia_gpu_db_stage_reserve": (C.c_int, [vp, C.c_size_t]),
        "uvaia_gpu_db_stage_packed": (C.c_int, [vp, C.c_int, C.c_void_p, pi, pi, C.c_int]),
        "uvaia_gpu_db_load_staged": (C.c_int, [vp, C.c_int, pi, C.c_int]),
        "uvaia_gpu_db_stage_packed_at": (C.c_int, [vp, C.c_int, C.c_size_t, C.c_void_p, pi, pi, C.c_int]),
        "uvaia_gpu_db_append_staged": (C.c_int, [vp, C.c_int, pi, C.c_int]),
        "uvaia_gpu_db_stage_compact_at": (C.c_int, [vp, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, pi, C.c_int]),
        "uvaia_gpu_compact_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_db_encode_compact": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, pi]),
        "uvaia_gpu_db_encoded_records": (C.c_int, [vp, C.c_void_p, C.c_void_p]),
        "uvaia_gpu_encode_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_db_unpack_rows": (C.c_int, [vp, pi, C.c_int, C.c_void_p, C.c_size_t]),
        "uvaia_gpu_window_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_db_stage_unpack_rows": (C.c_int, [vp, C.c_int, pi, C.c_int, C.c_void_p, C.c_size_t]),
        "uvaia_gpu_stage_unpack_ms": (C.c_double, [vp, C.c_int]),
        "uvaia_gpu_free_bytes": (C.c_size_t, [vp]),
        "uvaia_gpu_search_plan": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
        "uvaia_gpu_fasta_open": (C.c_int, [C.POINTER(vp), C.c_int, C.c_size_t, C.c_int]),
        "uvaia_gpu_fasta_close": (None, [vp]),
        "uvaia_gpu_fasta_last_error": (C.c_char_p, [vp]),
        "uvaia_gpu_fasta_scan": (C.c_int, [vp, C.c_void_p, C.c_size_t, C.c_int, pi, C.POINTER(C.c_size_t)]),
        "uvaia_gpu_fasta_bad": (C.c_uint, [vp, C.POINTER(C.c_size_t)]),
        "uvaia_gpu_fasta_records": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_fasta_rows": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), pi, pi]),
        "uvaia_gpu_fasta_rows_host": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_fasta_kernel_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_fasta_acgt": (C.c_int, [vp, pi]),
        "uvaia_gpu_fasta_sequences": (C.c_int, [vp, pi, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64)]),
        "uvaia_gpu_fasta_sequences_host": (C.c_int, [vp, C.c_void_p, C.c_size_t]),
        "uvaia_gpu_fasta_sequences_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_fasta_chunk_bytes": (C.c_size_t, []),
        "uvaia_gpu_fasta_pinned_alloc": (vp, [C.c_size_t]),
        "uvaia_gpu_fasta_pinned_free": (None, [vp]),
        "uvaia_gpu_text_append_device": (C.c_int, [vp, C.c_void_p, C.c_size_t, pi, C.c_int]),
        "uvaia_gpu_text_size": (C.c_size_t, [vp]),
        "uvaia_gpu_text_rows": (C.c_int, [vp, pi, C.c_int, C.c_void_p, C.c_size_t]),
        "uvaia_gpu_text_clear": (C.c_int, [vp]),
        "uvaia_gpu_text_reserve": (C.c_int, [vp, C.c_size_t]),
        "uvaia_gpu_text_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_db_pairs": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]),
        "uvaia_gpu_db_pairs_within": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]),
        "uvaia_gpu_pairs_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_db_link_begin": (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, C.c_int]),
        "uvaia_gpu_db_link": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_ulonglong)]),
        "uvaia_gpu_db_link_labels": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_link_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_db_near_begin": (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int]),
        "uvaia_gpu_db_near_components": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_db_near": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_ulonglong)]),
        "uvaia_gpu_db_near_fetch": (C.c_int, [vp, C.c_void_p]),
        "uvaia_gpu_db_mst": (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
        "uvaia_gpu_near_ms": (None, [vp, C.POINTER(C.c_double), C.c_int]),
        "uvaia_gpu_near_tiles": (None, [vp, C.POINTER(C.c_ulonglong), C.c_int]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def _cstrs(strs):
    arr = (C.c_char_p * len(strs))()
    for i, s in enumerate(strs):
        arr[i] = s
    return arr


def _int_ptr(a):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(a, dtype=np.int32)
    return arr, arr.ctypes.data_as(C.POINTER(C.c_int))


class Engine:
    """One GPU context over a prepared query set (fields of struct query_struct, src/fastaseq.h:41-48)."""

    def __init__(self, seqs, consensus, idx_c, idx_m, idx, trim=0, acgt=False, nbest=100, max_pool=4096, device=-1, tuning=None):
        self.L = load_library()
        self.nq, self.nchar = len(seqs), len(consensus)
        self._keep = [_cstrs(seqs), consensus,
                      (C.c_size_t * len(idx_c))(*[int(x) for x in idx_c]),
                      (C.c_size_t * len(idx_m))(*[int(x) for x in idx_m]),
                      (C.c_size_t * len(idx))(*[int(x) for x in idx])]
        q = _Query(self.nq, self.nchar, self._keep[0], consensus, self._keep[2], self._keep[3], self._keep[4],
                   len(idx_c), len(idx_m), len(idx), int(trim), int(bool(acgt)))
        self.ctx = C.c_void_p()
        tn = Tuning.make(tuning)
        rc = self.L.uvaia_gpu_open_tuned(C.byref(self.ctx), C.byref(q), int(nbest), int(device), int(max_pool), C.byref(tn) if tn is not None else None)
        if rc != 0:
            msg = self.L.uvaia_gpu_last_error(None)
            self.ctx = None
            raise GpuError(rc, msg.decode() if msg else "?")
        self.slots = self.L.uvaia_gpu_heap_slots(self.ctx)
        self.ordinal = 0

    @classmethod
    def from_query(cls, q, **kw):
        """q: any object with seqs, consensus, idx_c, idx_m, idx, trim, acgt."""
        return cls(q.seqs, q.consensus, q.idx_c, q.idx_m, q.idx, trim=q.trim, acgt=q.acgt, **kw)

    def _chk(self, rc):
        if rc != 0:
            msg = self.L.uvaia_gpu_last_error(self.ctx)
            raise GpuError(rc, msg.decode() if msg else "?")

    def close(self):
        if getattr(self, "ctx", None):
            self.L.uvaia_gpu_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, refs, non_n=None, ordinal0=None):
        """One batch (= one pool of the reference) in stream order; returns the 'entered any heap' flags."""
        n = len(refs)
        if ordinal0 is None:
            ordinal0 = self.ordinal
        self.ordinal = ordinal0 + n
        entered = np.zeros(n, dtype=np.uint8)
        if n == 0:
            return entered
        _k, nn = _int_ptr(non_n)
        self._chk(self.L.uvaia_gpu_push(self.ctx, _cstrs(refs), nn, n, ordinal0, entered.ctypes.data_as(C.POINTER(C.c_uint8))))
        return entered

    def last_batch_scores(self, n):
        out = np.zeros((n, self.nq, NSCORE), dtype=np.int32)
        self._chk(self.L.uvaia_gpu_last_batch_scores(self.ctx, out.ctypes.data_as(C.POINTER(C.c_int)), n))
        return out

    def drain(self):
        """(n_items[q], max_incompatible[q], scores[q, slot, 6], ordinals[q, slot]) in heap layout (slot 0 unused)."""
        n = np.zeros(self.nq, dtype=np.int32)
        T = np.zeros(self.nq, dtype=np.int32)
        sc = np.zeros((self.nq, self.slots + 1, NSCORE), dtype=np.int32)
        od = np.zeros((self.nq, self.slots + 1), dtype=np.int64)
        pi = C.POINTER(C.c_int)
        self._chk(self.L.uvaia_gpu_drain(self.ctx, n.ctypes.data_as(pi), T.ctypes.data_as(pi), sc.ctypes.data_as(pi),
                                         od.ctypes.data_as(C.POINTER(C.c_int64))))
        return n, T, sc, od

    def reset(self):
        self.ordinal = 0
        self._chk(self.L.uvaia_gpu_reset(self.ctx))

    def db_reserve(self, n):
        self._chk(self.L.uvaia_gpu_db_reserve(self.ctx, int(n)))

    def db_append(self, refs, non_n=None):
        _k, nn = _int_ptr(non_n)
        self._chk(self.L.uvaia_gpu_db_append(self.ctx, _cstrs(refs), nn, len(refs)))

    def db_append_block(self, block, non_n=None):
        """block: uint8 array [n, pitch] (pitch >= nchar)."""
        block = np.ascontiguousarray(block, dtype=np.uint8)
        _k, nn = _int_ptr(non_n)
        self._chk(self.L.uvaia_gpu_db_append_block(self.ctx, block.ctypes.data, block.shape[1], nn, block.shape[0]))

    def db_size(self):
        return self.L.uvaia_gpu_db_size(self.ctx)

    @staticmethod
    def _device_block(rows, pitch=None, n=None):
        """(pointer, pitch, rows, keep-alive) of a block of rows in device memory: a CUDA/HIP torch.uint8 tensor [n, pitch] whose rows are
        contiguous (any row stride: a view of a wider tensor works), or a raw device pointer with its pitch (and n where it is needed)"""
        if hasattr(rows, "data_ptr"):
            import torch
            if rows.dtype != torch.uint8 or rows.dim() != 2 or not rows.is_cuda or (rows.shape[0] > 0 and rows.shape[1] > 1 and rows.stride(1) != 1):
                raise GpuError(-1, "rows must be a 2-d torch.uint8 tensor in device memory with contiguous rows")
            torch.cuda.current_stream(rows.device).synchronize()          # the engine reads them on a stream of its own
            return rows.data_ptr(), (rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]), rows.shape[0], rows
        if pitch is None:
            raise GpuError(-1, "a raw device pointer needs its pitch")
        return int(rows), int(pitch), n, None

    def rows_census(self, rows, pitch=None, n=None):
        """(non_n [n], n_exc [n]) of a block of rows in device memory: valid sites and exception records of every row"""
        ptr, pitch, n, _keep = self._device_block(rows, pitch, n)
        non_n, n_exc = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        self._chk(self.L.uvaia_gpu_rows_census(self.ctx, ptr, pitch, n, non_n.ctypes.data_as(C.POINTER(C.c_int)), n_exc.ctypes.data_as(C.POINTER(C.c_int))))
        return non_n, n_exc

    def db_append_device(self, rows, row_index=None, non_n=None, pitch=None, n=None):
        """appends rows row_index (None: all n) of a block in device memory to the resident database, without a copy of their text"""
        ptr, pitch, n, _keep = self._device_block(rows, pitch, n)
        _k1, ri = _int_ptr(row_index)
        _k2, nn = _int_ptr(non_n)
        self._chk(self.L.uvaia_gpu_db_append_device(self.ctx, ptr, pitch, ri, n if row_index is None else len(row_index), nn))

    def rows_exceptions(self, rows, n_exc, row_index=None, pitch=None, n=None):
        """(offsets uint64 [n_sel + 1], records uint32 [total, 2] = (pos, len << 8 | char)) of the selected rows; n_exc: their record counts
        as rows_census gave them (one per selected row)"""
        ptr, pitch, n, _keep = self._device_block(rows, pitch, n)
        n_sel = n if row_index is None else len(row_index)
        off = np.zeros(n_sel + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.asarray(n_exc, dtype=np.uint64))
        out = np.zeros((int(off[-1]), 2), dtype=np.uint32)
        _k1, ri = _int_ptr(row_index)
        self._chk(self.L.uvaia_gpu_rows_exceptions(self.ctx, ptr, pitch, ri, n_sel, off.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data))
        return off, out

    def db_drop_tiles(self, n_tiles):
        self._chk(self.L.uvaia_gpu_db_drop_tiles(self.ctx, int(n_tiles)))

    def rows_kernel_ms(self, reset=False):
        out = (C.c_double * 3)()
        self.L.uvaia_gpu_rows_kernel_ms(self.ctx, out, int(reset))
        return {"census": out[0], "gather": out[1], "exceptions": out[2]}

    # ---- all pairs of the resident database against each other
    def db_pairs(self, rows=None, cols=None, trim=0, what=PAIRS_SNP, out=None, ld=None):
        """counters of rows (first, n) against cols (first, n) of the resident database (None: all of it): int32 [n_rows, ld] snp distances
        (what = PAIRS_SNP) or [n_rows, ld, 5] counters (PAIRS_COUNTS); the columns of out between n_cols and ld are left as they are"""
        r0, nr = (0, self.db_size()) if rows is None else rows
        c0, nc = (0, self.db_size()) if cols is None else cols
        ld = nc if ld is None else ld
        shape = (nr, ld, PAIR_NCOUNT) if what == PAIRS_COUNTS else (nr, ld)
        if out is None:
            out = np.zeros(shape, dtype=np.int32)
        if out.dtype != np.int32 or not out.flags.c_contiguous or out.size < int(np.prod(shape)):
            raise GpuError(-1, "out must be a contiguous int32 array of at least %r" % (shape,))
        self._chk(self.L.uvaia_gpu_db_pairs(self.ctx, int(r0), int(nr), int(c0), int(nc), int(trim), int(what), out.ctypes.data, int(ld)))
        return out

    def db_pairs_within(self, max_dist, rows=None, cols=None, trim=0, metric=DIST_SNP, upper=True, cap=None, out=None):
        """(records of PAIR_DTYPE, n_found): the pairs of the rectangle within max_dist, sorted by (row, col); cap None: the list is grown
        until everything fits; otherwise out (or a fresh array) of cap records is handed in as it is and n_found may exceed it"""
        r0, nr = (0, self.db_size()) if rows is None else rows
        c0, nc = (0, self.db_size()) if cols is None else cols
        n = C.c_ulonglong()
        grow = cap is None
        cap = 1024 if grow else int(cap)
        while True:
            buf = out if out is not None else np.zeros(cap, dtype=PAIR_DTYPE)
            self._chk(self.L.uvaia_gpu_db_pairs_within(self.ctx, int(r0), int(nr), int(c0), int(nc), int(trim), int(metric), int(max_dist), int(bool(upper)),
                                                       buf.ctypes.data if buf.size else None, cap, C.byref(n)))
            if not grow or n.value <= cap:
                return (buf[:n.value] if grow else buf), n.value
            cap = int(n.value)

    def pairs_ms(self, reset=False):
        out = (C.c_double * 3)()
        self.L.uvaia_gpu_pairs_ms(self.ctx, out, int(reset))
        return {"rows": out[0], "dense": out[1], "within": out[2]}

    # ---- single-linkage clusters within a distance
    def db_link_begin(self, max_dist, trim=0, metric=DIST_SNP, min_compared=0):
        """every resident reference a cluster of its own; the links of db_link are the pairs with distance <= max_dist under metric over at
        least min_compared compared sites"""
        self._chk(self.L.uvaia_gpu_db_link_begin(self.ctx, int(trim), int(metric), int(max_dist), int(min_compared)))

    def db_link(self, rows=None, cols=None):
        """links the pairs row < col of rows (first, n) x cols (first, n) (None: all of the database); returns how many there were"""
        r0, nr = (0, self.db_size()) if rows is None else rows
        c0, nc = (0, self.db_size()) if cols is None else cols
        n = C.c_ulonglong(0)
        self._chk(self.L.uvaia_gpu_db_link(self.ctx, int(r0), int(nr), int(c0), int(nc), C.byref(n)))
        return int(n.value)

    def db_link_labels(self):
        """uint32 [db_size]: the smallest database position of every reference's cluster, by the links made so far"""
        labels = np.zeros(self.db_size(), dtype=np.uint32)
        self._chk(self.L.uvaia_gpu_db_link_labels(self.ctx, labels.ctypes.data if labels.size else None))
        return labels

    def link_ms(self, reset=False):
        out = C.c_double(0.)
        self.L.uvaia_gpu_link_ms(self.ctx, C.byref(out), int(reset))
        return float(out.value)

    # ---- closest reference of another component, minimum spanning forest
    def db_near_begin(self, trim=0, metric=DIST_SNP, min_compared=0):
        """every resident reference a component of its own, every key NEAR_NONE; an edge is a pair compared over at least min_compared sites"""
        self._chk(self.L.uvaia_gpu_db_near_begin(self.ctx, int(trim), int(metric), int(min_compared)))

    def db_near_components(self, comp=None):
        """comp: one uint32 per resident reference (None: every reference its own); every key back to NEAR_NONE"""
        if comp is not None:
            comp = np.ascontiguousarray(comp, dtype=np.uint32)
            if comp.shape != (self.db_size(),):
                raise GpuError(-1, "comp must hold one value per resident reference")
        self._chk(self.L.uvaia_gpu_db_near_components(self.ctx, comp.ctypes.data if comp is not None and comp.size else None))

    def db_near(self, rows=None, cols=None, stats=True):
        """lowers the keys of both ends of the counting pairs row < col of rows (first, n) x cols (first, n) (None: all of the database);
        returns (tile pairs walked, tile pairs skipped) of this call, or None with stats=False (a NULL stats)"""
        r0, nr = (0, self.db_size()) if rows is None else rows
        c0, nc = (0, self.db_size()) if cols is None else cols
        st = (C.c_ulonglong * 2)(0, 0)
        self._chk(self.L.uvaia_gpu_db_near(self.ctx, int(r0), int(nr), int(c0), int(nc), st if stats else None))
        return (int(st[0]), int(st[1])) if stats else None

    def db_near_fetch(self):
        """uint64 [db_size]: dist << 32 | position of every reference's closest reference of another component so far, or NEAR_NONE"""
        best = np.zeros(self.db_size(), dtype=np.uint64)
        self._chk(self.L.uvaia_gpu_db_near_fetch(self.ctx, best.ctypes.data if best.size else None))
        return best

    def db_mst(self, trim=0, metric=DIST_SNP, min_compared=0):
        """(records of EDGE_DTYPE sorted by (dist, a, b), rounds): the minimum spanning forest of the resident database"""
        edges = np.zeros(max(self.db_size() - 1, 0), dtype=EDGE_DTYPE)
        n, rounds = C.c_size_t(0), C.c_int(0)
        self._chk(self.L.uvaia_gpu_db_mst(self.ctx, int(trim), int(metric), int(min_compared), edges.ctypes.data if edges.size else None, C.byref(n), C.byref(rounds)))
        return edges[:n.value], int(rounds.value)

    def near_ms(self, reset=False):
        out = C.c_double(0.)
        self.L.uvaia_gpu_near_ms(self.ctx, C.byref(out), int(reset))
        return float(out.value)

    def near_tiles(self, reset=False):
        """(tile pairs walked, tile pairs skipped) by every db_near since the last reset, those of db_mst included"""
        out = (C.c_ulonglong * 2)(0, 0)
        self.L.uvaia_gpu_near_tiles(self.ctx, out, int(reset))
        return int(out[0]), int(out[1])

    def rows_set_run_cut(self, cut):
        self._chk(self.L.uvaia_gpu_rows_set_run_cut(self.ctx, int(cut)))

    # ---- text row store: the text of rows that came from device memory, kept on the device
    def text_append_device(self, rows, row_index=None, pitch=None, n=None):
        """appends rows row_index (None: all n) of a block in device memory to the text row store"""
        ptr, pitch, n, _keep = self._device_block(rows, pitch, n)
        _k1, ri = _int_ptr(row_index)
        self._chk(self.L.uvaia_gpu_text_append_device(self.ctx, ptr, pitch, ri, n if row_index is None else len(row_index)))

    def text_size(self):
        return int(self.L.uvaia_gpu_text_size(self.ctx))

    def text_rows(self, index, pitch=None, out=None):
        """uint8 [len(index), pitch] (pitch >= nchar, default nchar): store rows `index`, any order, repeats allowed; out: a C-contiguous
        uint8 array of at least len(index) * pitch bytes to write into"""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pitch = self.nchar if pitch is None else int(pitch)
        rows = np.zeros((len(idx), pitch), dtype=np.uint8) if out is None else out
        self._chk(self.L.uvaia_gpu_text_rows(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_int)), len(idx), rows.ctypes.data, pitch))
        return rows

    def text_clear(self):
        self._chk(self.L.uvaia_gpu_text_clear(self.ctx))

    def text_reserve(self, n_rows):
        self._chk(self.L.uvaia_gpu_text_reserve(self.ctx, int(n_rows)))

    def text_ms(self, reset=False):
        out = (C.c_double * 2)()
        self.L.uvaia_gpu_text_ms(self.ctx, out, int(reset))
        return {"in": out[0], "out": out[1]}

    def set_active_queries(self, q0, q1):
        self._chk(self.L.uvaia_gpu_set_active_queries(self.ctx, int(q0), int(q1)))

    def max_tolerance(self):
        v = C.c_int(0)
        self._chk(self.L.uvaia_gpu_max_tolerance(self.ctx, C.byref(v)))
        return v.value

    def search_resident_pool(self, first, n, ordinal0, snapshot=-1):
        self._chk(self.L.uvaia_gpu_search_resident_pool(self.ctx, int(first), int(n), int(ordinal0), int(snapshot)))

    def db_clear(self):
        self._chk(self.L.uvaia_gpu_db_clear(self.ctx))

    # ---- reference shards (several GPUs): see include/uvaia_gpu.h
    def db_set_shard(self, rank, world, piece_refs):
        self._chk(self.L.uvaia_gpu_db_set_shard(self.ctx, int(rank), int(world), int(piece_refs)))

    def shard_rows(self):
        return self.L.uvaia_gpu_shard_rows(self.ctx)

    def shard_scan(self, first, n, cnt_ptr, tmin_ptr, aux_ptr):
        self._chk(self.L.uvaia_gpu_shard_scan(self.ctx, int(first), int(n), C.c_void_p(cnt_ptr), C.c_void_p(tmin_ptr), C.c_void_p(aux_ptr)))

    def shard_aux_bytes(self, n_tiles):
        return int(self.L.uvaia_gpu_shard_aux_bytes(self.ctx, int(n_tiles)))

    def db_skip(self, n_ref):
        """the next n_ref references of the stream belong to other ranks' pieces"""
        self._chk(self.L.uvaia_gpu_db_skip(self.ctx, int(n_ref)))

    def shard_ipc_handles(self):
        """bytes that let another process map this context's packed planes and side rows (uvaia_gpu_shard_ipc_open there)"""
        buf = C.create_string_buffer(self.L.uvaia_gpu_shard_ipc_handle_bytes())
        self._chk(self.L.uvaia_gpu_shard_ipc_handles(self.ctx, buf))
        return buf.raw

    def shard_ipc_close(self):
        self._chk(self.L.uvaia_gpu_shard_ipc_close(self.ctx))

    def shard_ipc_open(self, rank, handles):
        self._chk(self.L.uvaia_gpu_shard_ipc_open(self.ctx, int(rank), C.c_char_p(bytes(handles))))

    def scan_wait(self):
        self._chk(self.L.uvaia_gpu_scan_wait(self.ctx))

    def replay_wait(self):
        self._chk(self.L.uvaia_gpu_replay_wait(self.ctx))

    def set_snapshot(self, v):
        self._chk(self.L.uvaia_gpu_set_snapshot(self.ctx, int(v)))

    SCANS, REPLAYS = 0, 1

    def mark(self, what, slot):
        self._chk(self.L.uvaia_gpu_mark(self.ctx, int(what), int(slot)))

    def stream_wait_mark(self, stream, slot):
        self._chk(self.L.uvaia_gpu_stream_wait_mark(self.ctx, C.c_void_p(stream), int(slot)))

    def wait_stream(self, what, stream):
        self._chk(self.L.uvaia_gpu_wait_stream(self.ctx, int(what), C.c_void_p(stream)))

    def shard_replay(self, cnt_ptr, tmin_ptr, aux_ptr, owner, first, n, ordinal0, q0, q1):
        self._chk(self.L.uvaia_gpu_shard_replay(self.ctx, C.c_void_p(cnt_ptr), C.c_void_p(tmin_ptr), C.c_void_p(aux_ptr), int(owner), int(first), int(n), int(ordinal0), int(q0), int(q1)))

    def db_rederive(self):
        """Rebuild the query-set-dependent planes of the whole resident database (asynchronous)."""
        self._chk(self.L.uvaia_gpu_db_rederive(self.ctx))

    def db_export(self, first_tile=0, n_tiles=None):
        """Packed interchange form of the resident database: (planes uint8 [n_tiles, tile_bytes], non_n int32 [n_tiles*64],
        side_rows int32 [n_tiles*64, row_ints])."""
        if n_tiles is None:
            n_tiles = (self.db_size() + 63) // 64 - first_tile
        tb, ri = self.L.uvaia_gpu_db_tile_bytes(self.ctx), self.L.uvaia_gpu_db_side_row_ints()
        planes = np.zeros((n_tiles, tb), dtype=np.uint8)
        non_n = np.zeros(n_tiles * 64, dtype=np.int32)
        side = np.zeros((n_tiles * 64, ri), dtype=np.int32)
        self._chk(self.L.uvaia_gpu_db_export(self.ctx, first_tile, n_tiles, planes.ctypes.data, non_n.ctypes.data_as(C.POINTER(C.c_int)),
                                             side.ctypes.data_as(C.POINTER(C.c_int))))
        return planes, non_n, side

    def db_append_packed(self, planes, non_n, side_rows, n_ref):
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        non_n = np.ascontiguousarray(non_n, dtype=np.int32)
        side_rows = np.ascontiguousarray(side_rows, dtype=np.int32)
        self._chk(self.L.uvaia_gpu_db_append_packed(self.ctx, planes.ctypes.data, non_n.ctypes.data_as(C.POINTER(C.c_int)),
                                                    side_rows.ctypes.data_as(C.POINTER(C.c_int)), int(n_ref)))

    def search_resident(self, pool, ordinal0=0, want_entered=True):
        ent, p = None, None
        if want_entered:
            ent = np.zeros(self.db_size(), dtype=np.uint8)
            p = ent.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self.L.uvaia_gpu_search_resident(self.ctx, int(pool), int(ordinal0), p))
        return ent

    def search_plan(self, first, n, pool):
        """uvaia_gpu_search_plan: (first uint64 [slices], length uint64 [slices], opens a pool uint8 [slices]) of the slices a resident
        search cuts references [first, first + n) into when it runs them in batches of pool; host arithmetic only"""
        ns = self.L.uvaia_gpu_search_plan(self.ctx, int(first), int(n), int(pool), None, None, None, 0)
        if ns < 0:
            self._chk(ns)
        sf, sn, ps = np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint8)
        if ns:
            got = self.L.uvaia_gpu_search_plan(self.ctx, int(first), int(n), int(pool), sf.ctypes.data, sn.ctypes.data, ps.ctypes.data, ns)
            if got != ns:
                self._chk(got if got < 0 else -1)
        return sf, sn, ps

    def sync(self):
        self._chk(self.L.uvaia_gpu_sync(self.ctx))

    def scan_stats(self, reset=False):
        ms, n, b = C.c_double(), C.c_longlong(), C.c_double()
        self._chk(self.L.uvaia_gpu_scan_stats(self.ctx, C.byref(ms), C.byref(n), C.byref(b), int(reset)))
        return ms.value, n.value, b.value

    # ---- ring mode (several GPUs): see include/uvaia_gpu.h
    def state_bytes(self):
        return self.L.uvaia_gpu_state_bytes(self.ctx)

    def state_export(self, ptr):
        self._chk(self.L.uvaia_gpu_state_export(self.ctx, C.c_void_p(ptr)))

    def state_import(self, ptr):
        self._chk(self.L.uvaia_gpu_state_import(self.ctx, C.c_void_p(ptr)))

    def slice_scan(self, first, n, buf):
        self._chk(self.L.uvaia_gpu_slice_scan(self.ctx, int(first), int(n), int(buf)))

    def slice_replay(self, buf, ordinal0, stripe_start):
        self._chk(self.L.uvaia_gpu_slice_replay(self.ctx, int(buf), int(ordinal0), int(bool(stripe_start))))

    def state_range_bytes(self, q0, q1):
        return self.L.uvaia_gpu_state_range_bytes(self.ctx, int(q0), int(q1))

    def state_export_range(self, ptr, q0, q1):
        self._chk(self.L.uvaia_gpu_state_export_range(self.ctx, C.c_void_p(ptr), int(q0), int(q1)))

    def state_import_range(self, ptr, q0, q1):
        self._chk(self.L.uvaia_gpu_state_import_range(self.ctx, C.c_void_p(ptr), int(q0), int(q1)))

    def slice_replay_range(self, buf, ordinal0, q0, q1, take_snapshot):
        self._chk(self.L.uvaia_gpu_slice_replay_range(self.ctx, int(buf), int(ordinal0), int(q0), int(q1), int(bool(take_snapshot))))

    def entered_flags(self, clear=False):
        ent = np.zeros(self.db_size(), dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_entered_flags(self.ctx, ent.ctypes.data_as(C.POINTER(C.c_uint8)), int(clear)))
        return ent

    def replay_stats(self, reset=False):
        """(admissions, on-demand evaluations, dense rescans) since the last reset."""
        out = (C.c_ulonglong * 3)()
        self._chk(self.L.uvaia_gpu_replay_stats(self.ctx, out, int(reset)))
        return int(out[0]), int(out[1]), int(out[2])

    def replay_timing(self, reset=False):
        """ticks of an engine built with -DREPLAY_TIMING (see include/uvaia_gpu.h); zeros otherwise"""
        out = (C.c_ulonglong * 12)()
        self._chk(self.L.uvaia_gpu_replay_timing(self.ctx, out, int(reset)))
        return [int(x) for x in out]

    def replay_tiles_opened(self, reset=False):
        """(query, tile) pairs the replay of the packed-plane scan opened since the last reset."""
        out = C.c_ulonglong(0)
        self._chk(self.L.uvaia_gpu_replay_tiles_opened(self.ctx, C.byref(out), int(reset)))
        return int(out.value)

    def set_query_tile(self, qt):
        self._chk(self.L.uvaia_gpu_set_query_tile(self.ctx, int(qt)))

    def scan_bytes_per_ref(self):
        return self.L.uvaia_gpu_scan_bytes_per_ref(self.ctx)

    def derived_bytes_per_ref(self):
        return self.L.uvaia_gpu_derived_bytes_per_ref(self.ctx)

    def scan_variant(self):
        return self.L.uvaia_gpu_scan_variant(self.ctx)

    def packed_bytes_per_ref(self):
        return self.L.uvaia_gpu_packed_bytes_per_ref(self.ctx)

    def agree_on_polymorphic(self, seqs):
        """uint8 [len(seqs), n_query]: 1 where a sequence and a query differ at no polymorphic column (redundancy test)."""
        out = np.zeros((len(seqs), self.nq), dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_agree_on_polymorphic(self.ctx, _cstrs(seqs), len(seqs), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def ball(self, refs, radius):
        md = np.zeros(len(refs), dtype=np.int32)
        self._chk(self.L.uvaia_gpu_ball(self.ctx, _cstrs(refs), len(refs), int(radius), md.ctypes.data_as(C.POINTER(C.c_int))))
        return md

    def ball_resident(self, radius, first=0, n=None, want=True):
        n = self.db_size() - first if n is None else n
        md = np.zeros(n, dtype=np.int32) if want else None
        self._chk(self.L.uvaia_gpu_ball_resident(self.ctx, int(first), int(n), int(radius), md.ctypes.data_as(C.POINTER(C.c_int)) if want else None))
        return md

    def ball_packed(self, planes, n_ref, radius):
        """Radius search over ceil(n_ref / 64) tiles of the packed interchange form (uint8 [n_tiles, tile_bytes], as db_export gives them)."""
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        tb = self.L.uvaia_gpu_db_tile_bytes(self.ctx)
        if planes.size < (int(n_ref) + 63) // 64 * tb:
            raise ValueError("%d references need %d bytes of tiles, got %d" % (n_ref, (int(n_ref) + 63) // 64 * tb, planes.size))
        md = np.zeros(int(n_ref), dtype=np.int32)
        self._chk(self.L.uvaia_gpu_ball_packed(self.ctx, planes.ctypes.data, int(n_ref), int(radius), md.ctypes.data_as(C.POINTER(C.c_int))))
        return md

    def unpack_rows(self, index):
        """Upper-case text of references index[] of the last ball_packed batch, as a list of bytes (exception runs not applied)."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pitch = (self.nchar + 15) // 16 * 16
        rows = np.zeros((max(len(idx), 1), pitch), dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_unpack_rows(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_int)), len(idx), rows.ctypes.data, pitch))
        return [rows[k, :self.nchar].tobytes() for k in range(len(idx))]

    # ---- windowed search over a packed database (see include/uvaia_gpu.h)
    def db_stage_reserve(self, n_tiles):
        self._chk(self.L.uvaia_gpu_db_stage_reserve(self.ctx, int(n_tiles)))

    def db_stage_packed(self, slot, planes, non_n, side_rows, n_tiles):
        """asynchronous copy of n_tiles whole tiles into staging slot 0 or 1; the arrays are kept alive until the slot is staged again"""
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        non_n = np.ascontiguousarray(non_n, dtype=np.int32)
        side_rows = np.ascontiguousarray(side_rows, dtype=np.int32)
        tb = self.L.uvaia_gpu_db_tile_bytes(self.ctx)
        if planes.size < int(n_tiles) * tb or non_n.size < int(n_tiles) * 64 or side_rows.size < int(n_tiles) * 64 * self.L.uvaia_gpu_db_side_row_ints():
            raise ValueError("arrays shorter than %d tiles" % n_tiles)
        if not hasattr(self, "_staged"):
            self._staged = {}
        self._staged[int(slot)] = (planes, non_n, side_rows)
        self._chk(self.L.uvaia_gpu_db_stage_packed(self.ctx, int(slot), planes.ctypes.data, non_n.ctypes.data_as(C.POINTER(C.c_int)),
                                                   side_rows.ctypes.data_as(C.POINTER(C.c_int)), int(n_tiles)))

    def db_load_staged(self, slot, sel, n_ref):
        """the resident database becomes references sel[0 .. n_ref) of the slot (None: the first n_ref)"""
        _k, sp = _int_ptr(sel)
        self._chk(self.L.uvaia_gpu_db_load_staged(self.ctx, int(slot), sp, int(n_ref)))

    def db_stage_packed_at(self, slot, tile_offset, planes, non_n, side_rows, n_tiles):
        """db_stage_packed for a piece of a slot: the tiles land at tile_offset (a piece at 0 starts the slot afresh)"""
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        non_n = np.ascontiguousarray(non_n, dtype=np.int32)
        side_rows = np.ascontiguousarray(side_rows, dtype=np.int32)
        tb = self.L.uvaia_gpu_db_tile_bytes(self.ctx)
        if planes.size < int(n_tiles) * tb or non_n.size < int(n_tiles) * 64 or side_rows.size < int(n_tiles) * 64 * self.L.uvaia_gpu_db_side_row_ints():
            raise ValueError("arrays shorter than %d tiles" % n_tiles)
        if not hasattr(self, "_staged_at"):
            self._staged_at = {}
        if int(tile_offset) == 0:
            self._staged_at[int(slot)] = []
        self._staged_at.setdefault(int(slot), []).append((planes, non_n, side_rows))
        self._chk(self.L.uvaia_gpu_db_stage_packed_at(self.ctx, int(slot), int(tile_offset), planes.ctypes.data, non_n.ctypes.data_as(C.POINTER(C.c_int)),
                                                      side_rows.ctypes.data_as(C.POINTER(C.c_int)), int(n_tiles)))

    def db_stage_compact_at(self, slot, tile_offset, base, head_idx, heads, lit_idx, lits, non_n, n_tiles):
        """db_stage_packed_at for a piece of a compact (version 2) packed database: base row, the n_tiles * 64 + 1 offsets of the staged lanes
        into the file's heads and lits sections (given from their start), the lanes' valid-site counts; the tiles are expanded in the slot"""
        base = np.ascontiguousarray(base, dtype=np.uint32)
        head_idx = np.ascontiguousarray(head_idx, dtype=np.uint64)
        lit_idx = np.ascontiguousarray(lit_idx, dtype=np.uint64)
        heads = np.ascontiguousarray(heads, dtype=np.uint32)
        lits = np.ascontiguousarray(lits, dtype=np.uint32)
        non_n = np.ascontiguousarray(non_n, dtype=np.int32)
        lanes = int(n_tiles) * 64
        if base.size * 4 * 64 != self.L.uvaia_gpu_db_tile_bytes(self.ctx) or head_idx.size < lanes + 1 or lit_idx.size < lanes + 1 or non_n.size < lanes:
            raise ValueError("arrays shorter than %d tiles" % n_tiles)
        if lanes and (heads.size < int(head_idx[lanes]) or lits.size < int(lit_idx[lanes]) * 4):
            raise ValueError("records shorter than the index says")
        if not hasattr(self, "_staged_at"):
            self._staged_at = {}
        if int(tile_offset) == 0:
            self._staged_at[int(slot)] = []
        self._staged_at.setdefault(int(slot), []).append((base, head_idx, heads, lit_idx, lits, non_n))
        self._chk(self.L.uvaia_gpu_db_stage_compact_at(self.ctx, int(slot), int(tile_offset), base.ctypes.data, head_idx.ctypes.data, heads.ctypes.data,
                                                       lit_idx.ctypes.data, lits.ctypes.data, non_n.ctypes.data_as(C.POINTER(C.c_int)), int(n_tiles)))

    def compact_ms(self, reset=False):
        """Device ms since the last reset of (expand_tiles_kernel, the side-row pass after it)."""
        out = (C.c_double * 2)()
        self.L.uvaia_gpu_compact_ms(self.ctx, out, int(reset))
        return tuple(out)

    def db_encode_compact(self, base, first_tile=0, n_tiles=None):
        """Count pass of the compact form of resident tiles against `base` (uint32, one reference's worth of planes in the file's
        [word group][plane][4] order): (head_idx uint64 [n_tiles*64 + 1], lit_idx uint64 [n_tiles*64 + 1], non_n int32 [n_tiles*64]).
        The offsets start at 0, literal offsets count words of 16 bytes; db_encoded_records() then gives the records."""
        if n_tiles is None:
            n_tiles = (self.db_size() + 63) // 64 - first_tile
        base = np.ascontiguousarray(base, dtype=np.uint32)
        if base.size * 4 * 64 != self.L.uvaia_gpu_db_tile_bytes(self.ctx):
            raise ValueError("the base is not one reference's worth of planes")
        lanes = int(n_tiles) * 64
        head_idx = np.zeros(lanes + 1, dtype=np.uint64)
        lit_idx = np.zeros(lanes + 1, dtype=np.uint64)
        non_n = np.zeros(max(lanes, 1), dtype=np.int32)
        self._encode_sizes = None
        self._chk(self.L.uvaia_gpu_db_encode_compact(self.ctx, int(first_tile), int(n_tiles), base.ctypes.data, head_idx.ctypes.data, lit_idx.ctypes.data,
                                                     non_n.ctypes.data_as(C.POINTER(C.c_int))))
        self._encode_sizes = (int(head_idx[lanes]), int(lit_idx[lanes]))
        return head_idx, lit_idx, non_n[:lanes]

    def db_encoded_records(self):
        """Emit pass of the plan db_encode_compact left: (heads uint32 [head_idx[-1]], lits uint32 [lit_idx[-1], 4])."""
        nh, nl = getattr(self, "_encode_sizes", None) or (0, 0)
        heads = np.zeros(nh, dtype=np.uint32)
        lits = np.zeros((nl, 4), dtype=np.uint32)
        self._chk(self.L.uvaia_gpu_db_encoded_records(self.ctx, heads.ctypes.data if nh else None, lits.ctypes.data if nl else None))
        return heads, lits

    def encode_ms(self, reset=False):
        """Device ms since the last reset of (count + prefix passes, emit pass) of the compact encoder."""
        out = (C.c_double * 2)()
        self.L.uvaia_gpu_encode_ms(self.ctx, out, int(reset))
        return tuple(out)

    def db_append_staged(self, slot, sel, n_ref):
        """references sel[0 .. n_ref) of the slot (None: the first n_ref) go behind the resident ones, at any database size"""
        _k, sp = _int_ptr(sel)
        self._chk(self.L.uvaia_gpu_db_append_staged(self.ctx, int(slot), sp, int(n_ref)))

    def db_unpack_rows(self, index, pitch=None):
        """Upper-case text of references index[] of the window loaded last, as a list of bytes (exception runs not applied)."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pitch = (self.nchar + 15) // 16 * 16 if pitch is None else int(pitch)
        rows = np.zeros((max(len(idx), 1), pitch), dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_db_unpack_rows(self.ctx, idx.ctypes.data_as(C.POINTER(C.c_int)), len(idx), rows.ctypes.data, pitch))
        return [rows[k, :self.nchar].tobytes() for k in range(len(idx))]

    def db_stage_unpack_rows(self, slot, index, pitch=None):
        """Upper-case text of lanes index[] of staging slot 0 or 1 (positions within the slot, as sel of db_load_staged), as a list of
        bytes (exception runs not applied); the resident database and the search state are not touched."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pitch = (self.nchar + 15) // 16 * 16 if pitch is None else int(pitch)
        rows = np.zeros((max(len(idx), 1), max(pitch, 1)), dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_db_stage_unpack_rows(self.ctx, int(slot), idx.ctypes.data_as(C.POINTER(C.c_int)), len(idx), rows.ctypes.data, pitch))
        return [rows[k, :self.nchar].tobytes() for k in range(len(idx))]

    def stage_unpack_ms(self, reset=False):
        """Device ms since the last reset of the decode kernel of db_stage_unpack_rows."""
        return float(self.L.uvaia_gpu_stage_unpack_ms(self.ctx, int(reset)))

    def window_ms(self, reset=False):
        """Device ms since the last reset of (selection, totals + checks + derived planes after it, decode)."""
        out = (C.c_double * 3)()
        self.L.uvaia_gpu_window_ms(self.ctx, out, int(reset))
        return tuple(out)

    def free_bytes(self):
        return int(self.L.uvaia_gpu_free_bytes(self.ctx))

    def ball_asked(self, reset=False):
        return int(self.L.uvaia_gpu_ball_asked(self.ctx, int(reset)))

    def query_table(self, which):
        """uvaia_gpu_export_query_table: the table as bytes (numpy uint8)"""
        n = C.c_size_t(0)
        self._chk(self.L.uvaia_gpu_export_query_table(self.ctx, int(which), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            self._chk(self.L.uvaia_gpu_export_query_table(self.ctx, int(which), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def db_derived(self, n_tiles):
        """uvaia_gpu_db_derived_export: (e, grp, poly, tot) of the first n_tiles tiles as the column-compressed scan reads them."""
        W4 = ((self.nchar + 31) // 32 + 3) // 4
        counts = self.query_table(10).view(np.int32)
        NG = int(counts[2]) + int(counts[3])
        e = np.zeros((n_tiles, W4, 64, 4), dtype=np.uint32)
        grp = np.zeros((n_tiles, W4, 64), dtype=np.uint32)
        poly = np.zeros((n_tiles, NG, 3, 64, 4), dtype=np.uint32)
        tot = np.zeros(n_tiles * 64, dtype=np.int32)
        self._chk(self.L.uvaia_gpu_db_derived_export(self.ctx, int(n_tiles), e.ctypes.data, grp.ctypes.data, poly.ctypes.data, tot.ctypes.data))
        return e, grp, poly, tot

    def ball_kernel_ms(self, reset=False):
        """Device ms since the last reset of (consensus pass, gather of the asked references, pair scan)."""
        out = (C.c_double * 3)()
        self.L.uvaia_gpu_ball_kernel_ms(self.ctx, out, int(reset))
        return tuple(out)


class FastaRecord(C.Structure):
    """uvaia_gpu_fasta_record"""
    _fields_ = [("name_off", C.c_uint32), ("name_len", C.c_uint32), ("body_off", C.c_uint32), ("body_len", C.c_uint32),
                ("seq_len", C.c_uint32), ("non_n", C.c_int32), ("flags", C.c_uint32), ("bad_off", C.c_uint32)]

    def astuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


FASTA_RECORD_DTYPE = np.dtype([(f, np.int32 if f == "non_n" else np.uint32) for f, _ in FastaRecord._fields_])


class Fasta:
    """The FASTA parser's handle (uvaia_gpu_fasta): text in host memory split into records and rows on the device."""

    def __init__(self, block_bytes, max_records, device=-1):
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.uvaia_gpu_fasta_open(C.byref(self.h), int(device), int(block_bytes), int(max_records))
        if rc != 0:
            msg = self.L.uvaia_gpu_fasta_last_error(None)
            self.h = None
            raise GpuError(rc, msg.decode() if msg else "?")
        self.n_records = 0

    def _chk(self, rc):
        if rc != 0:
            raise GpuError(rc, self.L.uvaia_gpu_fasta_last_error(self.h).decode())

    def scan(self, text, final, offset=0):
        """text: bytes-like or a uint8 array whose bytes from `offset` on are the block; (n_records, consumed)"""
        arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
        n, cons = C.c_int(0), C.c_size_t(0)
        self.n_records = 0
        self._chk(self.L.uvaia_gpu_fasta_scan(self.h, arr.ctypes.data + int(offset), arr.size - int(offset), int(bool(final)), C.byref(n), C.byref(cons)))
        self.n_records = n.value
        return n.value, cons.value

    def bad(self):
        """(kind, offset) of what the last scan refused; kind 0: nothing of the text"""
        off = C.c_size_t(0)
        return int(self.L.uvaia_gpu_fasta_bad(self.h, C.byref(off))), off.value

    def records(self):
        """the table of the last scan as a structured array (FASTA_RECORD_DTYPE)"""
        out = np.zeros(self.n_records, dtype=FASTA_RECORD_DTYPE)
        self._chk(self.L.uvaia_gpu_fasta_records(self.h, out.ctypes.data))
        return out

    def rows(self, nchar):
        """pass 2: (device pointer, pitch, n_rows, row_of_record)"""
        p, pitch, n = C.c_void_p(), C.c_size_t(0), C.c_int(0)
        row_of = np.full(max(self.n_records, 1), -2, dtype=np.int32)
        self._chk(self.L.uvaia_gpu_fasta_rows(self.h, int(nchar), C.byref(p), C.byref(pitch), C.byref(n), row_of.ctypes.data_as(C.POINTER(C.c_int))))
        return p.value, pitch.value, n.value, row_of[:self.n_records]

    def rows_host(self, n_rows, pitch):
        out = np.zeros((n_rows, pitch), dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_fasta_rows_host(self.h, out.ctypes.data))
        return out

    def kernel_ms(self, reset=False):
        out = (C.c_double * 2)()
        self.L.uvaia_gpu_fasta_kernel_ms(self.h, out, int(reset))
        return list(out)

    def acgt(self):
        """per record of the last scan, its A C G T sites (upper or lower case)"""
        out = np.zeros(max(self.n_records, 1), dtype=np.int32)
        self._chk(self.L.uvaia_gpu_fasta_acgt(self.h, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out[:self.n_records]

    def sequences(self, record=None, n_sel=None):
        """the cleaned sequences of the records `record` (None: the first n_sel, or all) back to back: (device pointer, offsets [n_sel + 1])"""
        sel = None if record is None else np.ascontiguousarray(record, dtype=np.int32)
        n = int(len(sel) if sel is not None else (self.n_records if n_sel is None else n_sel))
        p, off = C.c_void_p(), np.zeros(n + 1, dtype=np.int64)
        self._chk(self.L.uvaia_gpu_fasta_sequences(self.h, None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_int)), n, C.byref(p), off.ctypes.data_as(C.POINTER(C.c_int64))))
        return p.value or 0, off

    def sequences_host(self, n_bytes):
        """the buffer of the last sequences(): n_bytes of sequences, then the 64 guard bytes, as (bytes, guard)"""
        out = np.zeros(int(n_bytes) + 64, dtype=np.uint8)
        self._chk(self.L.uvaia_gpu_fasta_sequences_host(self.h, out.ctypes.data, out.size))
        return out[:int(n_bytes)].tobytes(), out[int(n_bytes):]

    def sequences_ms(self, reset=False):
        out = (C.c_double * 2)()
        self.L.uvaia_gpu_fasta_sequences_ms(self.h, out, int(reset))
        return list(out)

    def close(self):
        if self.h:
            self.L.uvaia_gpu_fasta_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def finalise_heaps(n, scores, ordinals):
    """heap_finalise_heap_qsort (src/min_heap.c:149-158) on drained heaps: per query the rows best-first.

    The reference moves slots [1..n] to [0..n-1] by swapping slot 0 with slot n and then calls glibc qsort, which is
    a stable merge sort; a stable sort over that exact starting order gives the same table on any libc."""
    out = []
    for q in range(len(n)):
        k = int(n[q])
        order = ([k] + list(range(1, k))) if k else []          # slot n moved to position 0
        rows = [(tuple(int(x) for x in scores[q, s]), int(ordinals[q, s])) for s in order]
        rows.sort(key=lambda r: tuple(-v for v in r[0]))        # list.sort is stable
        out.append(rows)
    return out


class Group:
    """Several contexts driven from one host thread (uvaia_gpu_group_*): the reference-shard search with peer copies as the exchange."""

    def __init__(self, q, devices, nbest=100, max_pool=4096, piece_refs=0):
        self.L = load_library()
        self.nq, self.nchar = len(q.seqs), len(q.consensus)
        self._keep = [_cstrs(q.seqs), q.consensus,
                      (C.c_size_t * len(q.idx_c))(*[int(x) for x in q.idx_c]),
                      (C.c_size_t * len(q.idx_m))(*[int(x) for x in q.idx_m]),
                      (C.c_size_t * len(q.idx))(*[int(x) for x in q.idx])]
        qq = _Query(self.nq, self.nchar, self._keep[0], q.consensus, self._keep[2], self._keep[3], self._keep[4],
                    len(q.idx_c), len(q.idx_m), len(q.idx), int(q.trim), int(bool(q.acgt)))
        self.g = C.c_void_p()
        dev = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = self.L.uvaia_gpu_group_open(C.byref(self.g), C.byref(qq), int(nbest), dev, len(devices), int(max_pool), int(piece_refs))
        if rc != 0:
            msg = self.L.uvaia_gpu_group_last_error(None)
            self.g = None
            raise GpuError(rc, msg.decode() if msg else "?")
        self.slots = self.L.uvaia_gpu_heap_slots(self.L.uvaia_gpu_group_member(self.g, 0))

    def _chk(self, rc):
        if rc != 0:
            msg = self.L.uvaia_gpu_group_last_error(self.g)
            raise GpuError(rc, msg.decode() if msg else "?")

    def close(self):
        if getattr(self, "g", None):
            self.L.uvaia_gpu_group_close(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def query_shard(self, i):
        a, b = C.c_int(), C.c_int()
        self._chk(self.L.uvaia_gpu_group_query_shard(self.g, i, C.byref(a), C.byref(b)))
        return a.value, b.value

    def member_bytes_per_ref(self):
        """(packed planes, planes derived for the query set without V) bytes per reference a member keeps for its own pieces"""
        self.L.uvaia_gpu_packed_bytes_per_ref.restype = C.c_size_t
        self.L.uvaia_gpu_derived_bytes_per_ref.restype = C.c_size_t
        m0 = C.c_void_p(self.L.uvaia_gpu_group_member(self.g, 0))
        return int(self.L.uvaia_gpu_packed_bytes_per_ref(m0)), int(self.L.uvaia_gpu_derived_bytes_per_ref(m0))

    def db_reserve(self, n):
        self._chk(self.L.uvaia_gpu_group_db_reserve(self.g, int(n)))

    def db_append(self, refs, non_n=None):
        _k, nn = _int_ptr(non_n)
        self._chk(self.L.uvaia_gpu_group_db_append(self.g, _cstrs(refs), nn, len(refs)))

    def db_rederive(self):
        self._chk(self.L.uvaia_gpu_group_db_rederive(self.g))

    def reset(self):
        self._chk(self.L.uvaia_gpu_group_reset(self.g))

    def sync(self):
        self._chk(self.L.uvaia_gpu_group_sync(self.g))

    def search_resident(self, pool, ordinal0=0, want_entered=True):
        ent, p = None, None
        if want_entered:
            ent = np.zeros(self.L.uvaia_gpu_group_db_size(self.g), dtype=np.uint8)
            p = ent.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self.L.uvaia_gpu_group_search_resident(self.g, int(pool), int(ordinal0), p))
        return ent

    def push(self, refs, non_n=None, ordinal0=0):
        entered = np.zeros(len(refs), dtype=np.uint8)
        _k, nn = _int_ptr(non_n)
        self._chk(self.L.uvaia_gpu_group_push(self.g, _cstrs(refs), nn, len(refs), int(ordinal0), entered.ctypes.data_as(C.POINTER(C.c_uint8))))
        return entered

    def drain(self):
        n = np.zeros(self.nq, dtype=np.int32)
        T = np.zeros(self.nq, dtype=np.int32)
        sc = np.zeros((self.nq, self.slots + 1, NSCORE), dtype=np.int32)
        od = np.zeros((self.nq, self.slots + 1), dtype=np.int64)
        pi = C.POINTER(C.c_int)
        self._chk(self.L.uvaia_gpu_group_drain(self.g, n.ctypes.data_as(pi), T.ctypes.data_as(pi), sc.ctypes.data_as(pi), od.ctypes.data_as(C.POINTER(C.c_int64))))
        return n, T, sc, od


def query_columns(seqs, trim=0, acgt=False, device=-1):
    """create_query_indices' column walk on the device (uvaia_gpu_query_columns): (consensus bytes, some_missing uint8 array)."""
    L = load_library()
    n, nchar = len(seqs), len(seqs[0])
    arr = (C.c_char_p * n)(*seqs)
    cons = C.create_string_buffer(nchar)
    miss = np.zeros(nchar, dtype=np.uint8)
    rc = L.uvaia_gpu_query_columns(arr, n, nchar, int(trim), int(bool(acgt)), int(device), cons, miss.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        raise GpuError(rc, (L.uvaia_gpu_last_error(None) or b"").decode())
    return cons.raw[:nchar], miss
