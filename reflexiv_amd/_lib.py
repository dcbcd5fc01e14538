"""ctypes binding of libreflexiv_hip.so (include/reflexiv_hip.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 GPU is
present when a context is created, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libreflexiv_hip.so")
_LIB = None

RFX_OK, RFX_E_ARG, RFX_E_CAP, RFX_E_HIP, RFX_E_NOGPU, RFX_E_STATE, RFX_E_LIMIT, RFX_E_HOST = 0, -1, -2, -3, -4, -5, -6, -7
TWIN_DS, TWIN_RDD = 0, 1
_STATUS = {0: "RFX_OK", -1: "RFX_E_ARG", -2: "RFX_E_CAP", -3: "RFX_E_HIP", -4: "RFX_E_NOGPU",
           -5: "RFX_E_STATE", -6: "RFX_E_LIMIT", -7: "RFX_E_HOST"}


class RfxError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: {_STATUS.get(status, status)}{(' -- ' + detail) if detail else ''}")


class Params(C.Structure):
    """rfx_params (U/DefaultParam.java:74-120)."""
    _fields_ = [(n, C.c_int32) for n in (
        "k", "min_cov", "max_cov", "min_error_cov", "min_contig", "min_iter", "max_iter",
        "front_clip", "end_clip", "partitions", "twin", "coalesce", "extras")]


class CDynRecords(C.Structure):
    """rfx_dyn_records."""
    _fields_ = [("n", C.c_int64), ("key", C.c_void_p), ("key_off", C.c_void_p), ("ext", C.c_void_p), ("ext_off", C.c_void_p),
                ("marker", C.c_void_p), ("left", C.c_void_p), ("right", C.c_void_p), ("cap_n", C.c_int64), ("cap_key", C.c_int64),
                ("cap_ext", C.c_int64), ("need_key", C.c_int64), ("need_ext", C.c_int64)]


class CDynPacked(C.Structure):
    """rfx_dyn_packed: every pointer is a DEVICE pointer."""
    _fields_ = [("n", C.c_int64), ("key", C.c_void_p), ("key_len", C.c_void_p), ("ext", C.c_void_p), ("ext_off", C.c_void_p),
                ("ext_len", C.c_void_p), ("marker", C.c_void_p), ("left", C.c_void_p), ("right", C.c_void_p), ("cap_n", C.c_int64),
                ("cap_words", C.c_int64), ("need_words", C.c_int64)]


class CKsortParams(C.Structure):
    """rfx_ksort_params."""
    _fields_ = [("k", C.c_int), ("max_k", C.c_int), ("min_error_cov", C.c_int), ("max_cov", C.c_int), ("bubble", C.c_int),
                ("min_repeat_fold", C.c_double)]


class CReduceParams(C.Structure):
    """rfx_reduce_params."""
    _fields_ = [("k1", C.c_int), ("k2", C.c_int), ("max_k", C.c_int)]


class CReduceReadsParams(C.Structure):
    """rfx_reduce_reads_params."""
    _fields_ = [("min_cov", C.c_int), ("max_cov", C.c_int), ("min_error_cov", C.c_int), ("bubble", C.c_int), ("sensitive", C.c_int),
                ("front_clip", C.c_int), ("end_clip", C.c_int), ("P", C.c_int), ("min_repeat_fold", C.c_double)]


class CFixParams(C.Structure):
    """rfx_fix_params."""
    _fields_ = [("max_k", C.c_int), ("scramble", C.c_int), ("max_iteration", C.c_int)]


class CContigsPacked(C.Structure):
    """rfx_contigs_packed: every pointer is a DEVICE pointer."""
    _fields_ = [("n", C.c_int64), ("words", C.c_void_p), ("word_off", C.c_void_p), ("len", C.c_void_p), ("cap_n", C.c_int64),
                ("cap_words", C.c_int64), ("need_n", C.c_int64), ("need_words", C.c_int64)]


class CEndextConsensus(C.Structure):
    """rfx_endext_consensus: every pointer is a DEVICE pointer."""
    _fields_ = [("left", CContigsPacked), ("right", CContigsPacked), ("flags", C.c_void_p)]


class CEndextSet(C.Structure):
    """rfx_endext_set: every pointer is a DEVICE pointer."""
    _fields_ = [("set", CContigsPacked), ("left", C.c_void_p), ("right", C.c_void_p), ("left_len", C.c_void_p), ("right_len", C.c_void_p),
                ("flags", C.c_void_p), ("src_idx", C.c_void_p), ("new_idx", C.c_void_p)]


class CMapParams(C.Structure):
    """rfx_map_params."""
    _fields_ = [("seed", C.c_int), ("min_overlap", C.c_int), ("max_mismatch", C.c_int)]


class CMapHits(C.Structure):
    """rfx_map_hits: every pointer is a DEVICE pointer."""
    _fields_ = [("n", C.c_int64), ("read", C.c_void_p), ("end", C.c_void_p), ("strand", C.c_void_p), ("offset", C.c_void_p), ("v", C.c_void_p),
                ("cap_n", C.c_int64), ("need_n", C.c_int64), ("seed", C.c_int32)]


META_STAGES = ("00firstFour", "01Iteration5_9", "01Iteration10_14", "01Iteration15_19", "01Iteration21_30", "01Iteration31_40", "01Iteration41_50",
               "01Iteration51_60", "01Iteration61_70", "04Fixing", "05FixingAgain", "06ContigEnds", "Mapping", "07EndExtend", "08Extend", "09ExtendAgain",
               "Assembly")     # RFX_META_*: the values of rfx_meta_params.stop_after, in order


class CMetaParams(C.Structure):
    """rfx_meta_params."""
    _fields_ = [(n, C.c_int) for n in ("P", "scramble", "max_iteration", "min_contig", "map_seed", "map_min_overlap", "map_max_mismatch", "stop_after")]


class CMetaReport(C.Structure):
    """rfx_meta_report."""
    _fields_ = [("n_reduced", C.c_int64), ("n", C.c_int64 * len(META_STAGES)), ("hits", C.c_int64)]


class CRecords(C.Structure):
    """rfx_records."""
    _fields_ = [("n", C.c_int64), ("key", C.c_void_p), ("marker", C.c_void_p), ("ext_off", C.c_void_p),
                ("ext", C.c_void_p), ("left", C.c_void_p), ("right", C.c_void_p),
                ("cap_n", C.c_int64), ("cap_words", C.c_int64), ("need_n", C.c_int64), ("need_words", C.c_int64),
                ("key_words", C.c_int32), ("reserved_", C.c_int32)]


# every symbol include/reflexiv_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "rfx_version", "rfx_default_params", "rfx_ctx_create", "rfx_ctx_destroy", "rfx_ctx_sync",
    "rfx_ctx_set_stream", "rfx_ctx_stream", "rfx_last_error", "rfx_ctx_trim", "rfx_ctx_workspace_bytes",
    "rfx_extract_canon", "rfx_count_filter", "rfx_rc_expand_subkmer", "rfx_sort_records",
    "rfx_fork_filter_forward", "rfx_reflect_from_forward", "rfx_fork_filter_reflected",
    "rfx_random_reflection", "rfx_extend_pass", "rfx_contigs_text",
    "rfx_dev_encode_reads", "rfx_kmers_per_read", "rfx_count_workspace_bytes", "rfx_dev_count_reads",
    "rfx_dev_count_kmers", "rfx_dev_bucket_by_owner", "rfx_dev_bucket_records_by_owner",
    "rfx_dev_count_records", "rfx_dev_assemble", "rfx_dev_synth_genome",
    "rfx_dev_synth_reads", "rfx_dev_sort_pairs", "rfx_last_count_timing",
    "rfx_extract_canon_w", "rfx_count_filter_w", "rfx_kmers_per_read_w", "rfx_dev_count_reads_w",
    "rfx_dev_count_reads_ragged", "rfx_dev_count_reads_ragged_w", "rfx_assemble_reads", "rfx_dev_bucket_wide_by_owner", "rfx_dev_count_wide_elems",
    "rfx_dev_combine_reads", "rfx_dev_bucket_pairs_by_owner", "rfx_dev_merge_pairs",
    "rfx_dev_bucket_wide_records_by_owner", "rfx_dev_count_wide_records",
    "rfx_extras_operator", "rfx_assemble_counts_w", "rfx_dev_rc_expand_subkmer", "rfx_dev_sort_records", "rfx_dev_fork_filter",
    "rfx_dev_reflect_from_forward", "rfx_dev_random_reflection", "rfx_dev_extend_pass", "rfx_dev_lower_bound", "rfx_extend_pass_w", "rfx_dev_counter_to_asm", "rfx_dev_assemble_w", "rfx_dev_order_kmers_w",
    "rfx_comm_unique_id", "rfx_comm_init", "rfx_comm_destroy", "rfx_comm_rank", "rfx_comm_world", "rfx_comm_last_bytes_bucketed",
    "rfx_comm_all_reduce_i64", "rfx_dev_sharded_count", "rfx_dev_gather_shards", "rfx_sharded_assemble_reads", "rfx_dev_sharded_assemble",
    "rfx_dedup_contigs", "rfx_dedup_contig_text",
    "rfx_dev_contigs_pack", "rfx_dev_contigs_unpack", "rfx_dev_contigs_from_text", "rfx_dev_contigs_to_text", "rfx_dev_dedup_contigs",
    "rfx_dyn_binarize", "rfx_dyn_sort", "rfx_dyn_random_reflection", "rfx_dyn_extend_pass", "rfx_dyn_run",
    "rfx_dyn_blocks_to_bases", "rfx_dyn_bases_to_blocks", "rfx_dyn_attribute", "rfx_dyn_attribute_unpack",
    "rfx_dev_dyn_pack", "rfx_dev_dyn_unpack", "rfx_dev_dyn_binarize", "rfx_dev_dyn_sort", "rfx_dev_dyn_random_reflection",
    "rfx_dev_dyn_extend_pass", "rfx_dev_dyn_run", "rfx_dev_dyn_to_text", "rfx_dyn_run_text",
    "rfx_ksort_default_params", "rfx_dev_ksort_binarize", "rfx_dev_ksort_fork_filter", "rfx_dev_ksort_reflect",
    "rfx_dev_ksort_full_kmers", "rfx_dev_ksort_to_text", "rfx_dev_ksort_run", "rfx_ksort_text",
    "rfx_dev_ksort_from_counts", "rfx_dev_ksort_run_counts", "rfx_dev_reduce_union_packed", "rfx_dev_reduce_run_packed",
    "rfx_dev_dyn_from_kmers", "rfx_reduce_reads_default_params", "rfx_dev_reduce_reads", "rfx_reduce_reads",
    "rfx_reduce_default_params", "rfx_dev_reduce_union", "rfx_dev_reduce_left_prepare", "rfx_dev_reduce_adjust",
    "rfx_dev_reduce_right_prepare", "rfx_dev_reduce_full_kmers", "rfx_dev_reduce_neutralize", "rfx_dev_reduce_run", "rfx_reduce_text",
    "rfx_fix_default_params", "rfx_dev_fix_binarize", "rfx_dev_fix_contig_ends", "rfx_dev_fix_kmer_set", "rfx_dev_fix_fork_filter",
    "rfx_dev_fix_reflect", "rfx_dev_fix_run", "rfx_fix_text", "rfx_dev_fix_run_packed",
    "rfx_dev_fix2_binarize", "rfx_dev_fix2_run", "rfx_dev_fix2_contigs", "rfx_dev_fix2_to_text", "rfx_dev_fix2_ends_text", "rfx_fix2_text",
    "rfx_dev_endext_consensus", "rfx_dev_endext_consensus_hits", "rfx_dev_endext_contigs", "rfx_dev_endext_to_text", "rfx_endext_text",
    "rfx_dev_ext_from_text", "rfx_dev_ext_contig_ends", "rfx_dev_ext_run", "rfx_ext_text", "rfx_dev_ext2_to_text", "rfx_ext2_text",
    "rfx_map_default_params", "rfx_dev_map_ends", "rfx_dev_map_to_text", "rfx_map_text",
    "rfx_dev_mercy_kmers", "rfx_dev_mercy_to_text", "rfx_mercy_text",
    "rfx_meta_default_params", "rfx_dev_meta_from_reduced", "rfx_dev_meta_reads", "rfx_meta_reads",
]

# prototypes of the packed entry points (ctx, then as include/reflexiv_hip.h declares them)
_PK, _HR, _CP, _KP, _RP, _FP, _I, _L, _P = "PK", "HR", "CP", "KP", "RP", "FP", C.c_int, C.c_int64, C.c_void_p
_EC, _ES, _MP, _MH, _RR, _MT, _MR = "EC", "ES", "MP", "MH", "RR", "MT", "MR"
_DYN_PACKED_ARGS = {
    "rfx_dev_dyn_pack": (_HR, _PK),
    "rfx_dev_dyn_unpack": (_PK, _HR),
    "rfx_dev_dyn_binarize": (_P, _P, _L, _I, _PK),
    "rfx_dev_dyn_sort": (_PK, _I, _PK, _P),
    "rfx_dev_dyn_random_reflection": (_PK, _P, _I, _PK),
    "rfx_dev_dyn_extend_pass": (_PK, _P, _I, _I, _I, _I, _PK, _P),
    "rfx_dev_dyn_run": (_PK, _I, _I, _I, _I, _I, _PK, _P, _L, _P),
    "rfx_dev_dyn_to_text": (_PK, _P, _L, _P),
    "rfx_dyn_run_text": (_P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _L, _P, _P, _L, _P),
    # the k-mer sorting stage on the same packed sets (rfx_ksort_params)
    "rfx_dev_ksort_binarize": (_P, _P, _L, _KP, _PK),
    "rfx_dev_ksort_fork_filter": (_I, _PK, _KP, _PK),
    "rfx_dev_ksort_reflect": (_PK, _PK),
    "rfx_dev_ksort_full_kmers": (_PK, _PK),
    "rfx_dev_ksort_to_text": (_PK, _I, _P, _L, _P, _P, _P),
    "rfx_dev_ksort_run": (_P, _P, _L, _KP, _PK),
    "rfx_ksort_text": (_P, _P, _L, _KP, _P, _L, _P),
    "rfx_dev_ksort_from_counts": (_P, _P, _I, _L, _P, _L, _KP, _PK),
    "rfx_dev_ksort_run_counts": (_P, _P, _I, _L, _P, _L, _KP, _PK),
    # the packed seams of the reduction: two packed sets in, and an array of packed sets with one key length each
    "rfx_dev_reduce_union_packed": (_PK, _PK, _RP, _PK),
    "rfx_dev_reduce_run_packed": (_PK, _PK, _I, _RP, _PK),
    "rfx_dev_dyn_from_kmers": (_P, _P, _I, _PK),
    # the driver from reads: the read store and the k list in, the set of the first-four passes and each k's row count out
    "rfx_dev_reduce_reads": (_P, _P, _L, _I, _I, _P, _I, _RR, _PK, _P),
    "rfx_reduce_reads": (_P, _P, _L, _P, _I, _RR, _P, _L, _P, _P),
    # the k-mer reduction stage on the same packed sets (rfx_reduce_params)
    "rfx_dev_reduce_union": (_P, _P, _L, _P, _P, _L, _RP, _PK),
    "rfx_dev_reduce_left_prepare": (_PK, _RP, _PK),
    "rfx_dev_reduce_adjust": (_I, _PK, _P, _I, _RP, _PK, _P),
    "rfx_dev_reduce_right_prepare": (_PK, _RP, _PK),
    "rfx_dev_reduce_full_kmers": (_PK, _RP, _PK),
    "rfx_dev_reduce_neutralize": (_PK, _P, _I, _RP, _PK, _P),
    "rfx_dev_reduce_run": (_P, _P, _L, _P, _P, _L, _I, _RP, _PK),
    "rfx_reduce_text": (_P, _P, _L, _P, _P, _L, _I, _RP, _P, _L, _P, _P, _L, _P),
    # the contig fixing stage on the same packed sets (rfx_fix_params)
    "rfx_dev_fix_binarize": (_P, _P, _L, _FP, _PK),
    "rfx_dev_fix_contig_ends": (_PK, _FP, _PK, _P, _L, _P),
    "rfx_dev_fix_kmer_set": (_P, _L, _PK, _PK),
    "rfx_dev_fix_fork_filter": (_I, _PK, _P, _I, _PK, _P),
    "rfx_dev_fix_reflect": (_PK, _PK),
    "rfx_dev_fix_run": (_P, _P, _L, _I, _FP, _PK),
    "rfx_fix_text": (_P, _P, _L, _I, _FP, _P, _L, _P),
    "rfx_dev_fix_run_packed": (_PK, _I, _FP, _PK),
    # the second contig fixing stage: packed sets in, a packed contig set and the two texts out
    "rfx_dev_fix2_binarize": (_P, _P, _L, _PK),
    "rfx_dev_fix2_run": (_PK, _I, _FP, _PK),
    "rfx_dev_fix2_contigs": (_PK, _FP, _CP, _P, _P),
    "rfx_dev_fix2_to_text": (_CP, _P, _P, _P, _L, _P),
    "rfx_dev_fix2_ends_text": (_CP, _P, _P, _P, _L, _P),
    "rfx_fix2_text": (_P, _P, _L, _I, _FP, _P, _L, _P, _P, _L, _P),
    # the end extension from alignment rows: a packed contig set and rows in, consensus sets, the spliced set and its text out
    "rfx_dev_endext_consensus": (_CP, _P, _P, _P, _P, _L, _EC),
    "rfx_dev_endext_consensus_hits": (_CP, _P, _P, _P, _P, _I, _MH, _EC),
    "rfx_dev_endext_contigs": (_CP, _P, _P, _EC, _I, _ES),
    "rfx_dev_endext_to_text": (_ES, _P, _L, _P),
    "rfx_endext_text": (_P, _P, _L, _P, _P, _L, _I, _P, _L, _P),
    # the contig extension stages: the set of 07EndExtend in, the record set of 08Extend and the text of 09ExtendAgain out
    "rfx_dev_ext_from_text": (_P, _P, _L, _FP, _ES),
    "rfx_dev_ext_contig_ends": (_ES, _FP, _PK, _P, _L, _P),
    "rfx_dev_ext_run": (_ES, _I, _FP, _PK),
    "rfx_ext_text": (_P, _P, _L, _I, _FP, _P, _L, _P),
    "rfx_dev_ext2_to_text": (_CP, _P, _L, _P),
    "rfx_ext2_text": (_P, _P, _L, _I, _FP, _P, _L, _P),
    # reads onto the contig ends: a packed contig set and the read store in, the hits and their row text out
    "rfx_dev_map_ends": (_CP, _P, _P, _P, _P, _L, _I, _MP, _MH),
    "rfx_dev_map_to_text": (_CP, _P, _P, _P, _P, _I, _MH, _P, _L, _P, _P, _L),
    "rfx_map_text": (_P, _P, _L, _P, _P, _L, _MP, _P, _L, _P),
    # the mercy k-mer stage: the counter's solid keys and the read store in, the mercy k-mers and their row text out
    "rfx_dev_mercy_kmers": (_P, _L, _P, _P, _L, _I, _I, _I, _I, _P, _L, _P),
    "rfx_dev_mercy_to_text": (_P, _L, _I, _P, _L, _P, _P),
    "rfx_mercy_text": (_P, _P, _L, _P, _P, _L, _I, _I, _I, _P, _L, _P),
    # reads to contigs in one resident call: the read store (or ASCII reads) and the k list in, the contig set (or one stage's text) out
    "rfx_dev_meta_from_reduced": (_PK, _P, _P, _L, _I, _I, _MT, _MR, _CP),
    "rfx_dev_meta_reads": (_P, _P, _L, _I, _I, _P, _I, _RR, _MT, _MR, _CP),
    "rfx_meta_reads": (_P, _P, _L, _P, _I, _RR, _MT, _MR, _P, _L, _P),
    # the packed contig set of the de-duplication (rfx_contigs_packed)
    "rfx_dev_contigs_pack": (_P, _P, _L, _CP),
    "rfx_dev_contigs_unpack": (_CP, _P, _L, _P, _L, _P),
    "rfx_dev_contigs_from_text": (_P, _L, _CP),
    "rfx_dev_contigs_to_text": (_CP, _I, _P, _L, _P, _P),
    "rfx_dev_dedup_contigs": (_CP, _CP, _P),
}


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    host = os.path.join(src, "host")
    newest = max(os.path.getmtime(os.path.join(src, f)) for f in os.listdir(src)
                 if f.endswith((".hip", ".h")) or f == "Makefile")
    newest = max(newest, os.path.getmtime(os.path.join(_HERE, "..", "include", "reflexiv_hip.h")))
    newest_host = max([newest] + [os.path.getmtime(os.path.join(host, f)) for f in os.listdir(host)])
    built = [(LIB_PATH, newest), (os.path.join(_HERE, "reflexiv_host"), newest_host)]     # (make rebuilds what is behind its sources)
    if force or any(not os.path.exists(p) or os.path.getmtime(p) < t for p, t in built):
        subprocess.check_call(["make", "-s", "-j4", "-C", src])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RfxError(RFX_E_NOGPU, "reflexiv_amd",
                           f"{LIB_PATH} is missing -- build it with reflexiv_amd._lib.build() "
                           "(there is no CPU fallback)")
        # One HIP runtime per process: torch ships its own libamdhip64 (soname libamdhip64.so.7).
        # Loaded first, it also satisfies this library's NEEDED entry, so device pointers and
        # streams are shared with torch; loaded second, the process would hold two runtimes.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.rfx_version.restype = C.c_int
        L.rfx_ctx_stream.restype = C.c_void_p
        L.rfx_last_error.restype = C.c_char_p
        L.rfx_kmers_per_read.restype = C.c_int64
        L.rfx_count_workspace_bytes.restype = C.c_int64
        L.rfx_count_workspace_bytes.argtypes = [C.c_int64]
        for name in SYMBOLS:
            fn = getattr(L, name)
            if name == "rfx_kmers_per_read_w":
                fn.restype = C.c_int64
                continue
            if name == "rfx_dyn_attribute":
                fn.restype = C.c_int64
                fn.argtypes = [C.c_int, C.c_int, C.c_int]
                continue
            if name in _DYN_PACKED_ARGS:
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p] + [C.POINTER(CDynPacked) if a == _PK else C.POINTER(CDynRecords) if a == _HR else
                                              C.POINTER(CContigsPacked) if a == _CP else C.POINTER(CKsortParams) if a == _KP else C.POINTER(CReduceParams) if a == _RP else
                                              C.POINTER(CFixParams) if a == _FP else C.POINTER(CEndextConsensus) if a == _EC else
                                              C.POINTER(CEndextSet) if a == _ES else C.POINTER(CMapParams) if a == _MP else
                                              C.POINTER(CMapHits) if a == _MH else C.POINTER(CReduceReadsParams) if a == _RR else
                                              C.POINTER(CMetaParams) if a == _MT else C.POINTER(CMetaReport) if a == _MR else a for a in _DYN_PACKED_ARGS[name]]
                continue
            if name == "rfx_dyn_attribute_unpack":
                fn.restype = None
                continue
            if name == "rfx_ksort_default_params":
                fn.restype = None
                fn.argtypes = [C.POINTER(CKsortParams), C.c_int]
                continue
            if name == "rfx_reduce_default_params":
                fn.restype = None
                fn.argtypes = [C.POINTER(CReduceParams), C.c_int, C.c_int]
                continue
            if name == "rfx_fix_default_params":
                fn.restype = None
                fn.argtypes = [C.POINTER(CFixParams), C.c_int]
                continue
            if name == "rfx_reduce_reads_default_params":
                fn.restype = None
                fn.argtypes = [C.POINTER(CReduceReadsParams)]
                continue
            if name == "rfx_meta_default_params":
                fn.restype = None
                fn.argtypes = [C.POINTER(CMetaParams)]
                continue
            if name == "rfx_map_default_params":
                fn.restype = None
                fn.argtypes = [C.POINTER(CMapParams)]
                continue
            if name in ("rfx_comm_last_bytes_bucketed", "rfx_ctx_workspace_bytes"):
                fn.restype = C.c_int64
                fn.argtypes = [C.c_void_p]
                continue
            if name == "rfx_comm_destroy":
                fn.restype = None
                fn.argtypes = [C.c_void_p]
                continue
            if name not in ("rfx_ctx_stream", "rfx_last_error", "rfx_kmers_per_read",
                            "rfx_count_workspace_bytes", "rfx_ctx_destroy", "rfx_default_params"):
                fn.restype = C.c_int
        _LIB = L
    return _LIB
