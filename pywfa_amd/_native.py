"""ctypes binding of libwfa_hip.so (the C ABI declared in include/wfa_hip.h).

This is the reference-side binding a pywfa maintainer would add instead of ``WFA_wrap.pxd``
(INTEGRATION.md shows the Cython form).  There is NO CPU fallback: if the library cannot be loaded,
or no HIP device is present, every alignment entry point raises.
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WFA_HIP_LIB") or os.path.join(_HERE, "libwfa_hip.so")  # (WFA_HIP_LIB: development builds)

ABI_VERSION = 4

OK, EINVAL, ENOTSUP, EDEVICE = 0, -1, -2, -3

DIST = {"indel": 0, "levenshtein": 1, "linear": 2, "affine": 3, "affine2p": 4}
DIST_NAMES = {v: k for k, v in DIST.items()}
SCOPE = {"score": 0, "full": 1}
SPAN = {"end-to-end": 0, "ends-free": 1}
HEUR = {None: 0, "adaptive": 1, "X-drop": 2}
HEUR_NAMES = {v: k for k, v in HEUR.items()}
MEM = {"high": 0, "medium": 1, "low": 2, "biwfa": 3}
MEM_NAMES = {v: k for k, v in MEM.items()}


class Config(ctypes.Structure):
    """wfa_hip_config_t"""

    _fields_ = [(n, ctypes.c_int32) for n in (
        "distance", "match", "mismatch", "gap_opening", "gap_extension", "gap_opening2",
        "gap_extension2", "scope", "span", "pattern_begin_free", "pattern_end_free",
        "text_begin_free", "text_end_free", "heuristic", "min_wavefront_length",
        "max_distance_threshold", "steps_between_cutoffs", "xdrop", "memory_mode", "max_steps",
        "wildcard", "reserved")]

    def copy(self):
        c = Config()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(self), ctypes.sizeof(Config))
        return c


class NativeError(RuntimeError):
    pass


_lib = None

_int, _i32, _i64, _vp, _str, _size = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
_cfgp, _intp, _i64p, _floatp = (ctypes.POINTER(t) for t in (Config, ctypes.c_int, ctypes.c_int64, ctypes.c_float))
_CTYPES = object()   # a restype / argtypes that ``lib()`` leaves as ctypes has it (int; unchecked arguments)
_ALIGN_BATCH = [_vp, _i64] + [_vp] * 11
_BATCH_CREATE = [_vp, _i64] + [_vp] * 5
_INDEX_CREATE = [_vp, _vp, _int, _int, _int]
_SEEDS_HOST = [_vp, _i32, _i64, _vp, _vp, _vp] + [_int] * 8 + [_vp] * 6 + [_str, _size]
_CHAINS_HOST = [_vp, _i32, _i64, _vp, _vp, _vp] + [_int] * 11 + [_vp] * 9 + [_str, _size]
_HITS = [_i64, _i64] + [_vp] * 7   # nreads, the hits and their seven arrays (the host rules)

# every symbol include/wfa_hip.h declares (tests/test_abi.py checks the library exports them all): name -> (restype, argtypes)
SIGNATURES = {
    "wfa_hip_abi_version": (_int, _CTYPES),
    "wfa_hip_device_count": (_int, _CTYPES),
    "wfa_hip_global_error": (_str, _CTYPES),
    "wfa_hip_config_default": (_CTYPES, [_cfgp]),
    "wfa_hip_config_validate": (_CTYPES, [_cfgp, _str, _size]),
    "wfa_hip_create": (_vp, [_cfgp, _int]),
    "wfa_hip_destroy": (None, [_vp]),
    "wfa_hip_set_config": (_CTYPES, [_vp, _cfgp]),
    "wfa_hip_get_config": (_CTYPES, [_vp, _cfgp]),
    "wfa_hip_last_error": (_str, [_vp]),
    "wfa_hip_align_batch": (_CTYPES, _ALIGN_BATCH),
    "wfa_hip_batch_create": (_vp, _BATCH_CREATE),
    "wfa_hip_batch_destroy": (None, [_vp]),
    "wfa_hip_batch_run": (_CTYPES, [_vp, _vp]),
    "wfa_hip_batch_sync": (_CTYPES, [_vp]),
    "wfa_hip_batch_results": (_CTYPES, [_vp] * 7),
    "wfa_hip_batch_last_kernel_ms": (_CTYPES, [_vp, _floatp, _i64p]),
    "wfa_hip_batch_algorithmic_bytes": (_i64, [_vp]),
    "wfa_hip_batch_fallback_pairs": (_i64, [_vp]),
    "wfa_hip_batch_rle_counts": (_i64, [_vp, _vp, _vp]),
    "wfa_hip_batch_rle_runs": (_CTYPES, [_vp, _vp, _vp]),
    "wfa_hip_plan_shards": (_CTYPES, [_i64, _vp, _vp, _int, _vp]),
    "wfa_hip_plan_host_threads": (_CTYPES, [_int, _int, _intp, _intp]),
    "wfa_hip_multi_create": (_vp, [_cfgp, _vp, _int]),
    "wfa_hip_multi_destroy": (None, [_vp]),
    "wfa_hip_multi_set_config": (_CTYPES, [_vp, _cfgp]),
    "wfa_hip_multi_last_error": (_str, [_vp]),
    "wfa_hip_multi_align_batch": (_CTYPES, _ALIGN_BATCH),
    "wfa_hip_pack_2bit": (_CTYPES, [_vp, _i32, _vp, _int]),
    "wfa_hip_batch_extent": (_i64, [_i64, _vp, _vp, _vp, _vp]),
    "wfa_hip_align_batch_packed2bits": (_CTYPES, _ALIGN_BATCH),
    "wfa_hip_batch_create_packed2bits": (_vp, _BATCH_CREATE),
    "wfa_hip_cigar_sprint_pretty": (_i64, [_vp, _i64, _vp, _i32, _vp, _i32, _vp, _i64]),
    "wfa_hip_batch_extent_packed2bits": (_i64, [_i64, _vp, _vp, _vp, _vp]),
    "wfa_hip_align_pair": (_CTYPES, [_vp, _str, _i32, _str, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wfa_hip_upload_info": (_CTYPES, [_vp, _vp, _int]),
    "wfa_hip_seqset_create": (_vp, [_vp, _i64, _vp, _vp, _vp]),
    "wfa_hip_seqset_destroy": (None, [_vp]),
    "wfa_hip_cross_run": (_vp, [_vp, _vp, _vp, _int]),
    "wfa_hip_cross_dense": (_CTYPES, [_vp, _vp, _vp]),
    "wfa_hip_cross_completed": (_CTYPES, [_vp, _i64p, _vp, _vp, _vp]),
    "wfa_hip_cross_kernel_ms": (_CTYPES, [_vp, _floatp, _i64p]),
    "wfa_hip_cross_destroy": (None, [_vp]),
    "wfa_hip_plan_cross_bands": (_i64, [_i64, _i64, _int, _i64, _vp, _i64]),
    "wfa_hip_cross_run_k": (_vp, [_vp, _vp, _vp, _int, _int]),
    "wfa_hip_cross_topk": (_CTYPES, [_vp, _vp, _vp]),
    "wfa_hip_batch_create_indexed": (_vp, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "wfa_hip_batch_create_windows": (_vp, [_vp, _vp, _vp, _i64] + [_vp] * 7),
    "wfa_hip_window_2bit": (_CTYPES, [_vp, _i64, _i32, _int, _vp]),
    "wfa_hip_batch_summary": (_CTYPES, [_vp, _vp]),
    "wfa_hip_ops_summary": (_CTYPES, [_vp, _i64, _i32, _i32, _vp]),
    "wfa_hip_pileup_create": (_vp, [_vp, _vp]),
    "wfa_hip_pileup_add": (_CTYPES, [_vp, _vp, _vp, _vp, _vp]),
    "wfa_hip_pileup_read": (_CTYPES, [_vp, _i32, _i64, _i64, _vp]),
    "wfa_hip_pileup_clear": (_CTYPES, [_vp]),
    "wfa_hip_pileup_destroy": (None, [_vp]),
    "wfa_hip_ops_pileup": (_CTYPES, [_vp, _i64, _vp, _i32, _i32, _vp]),
    "wfa_hip_seed_index_create": (_vp, _INDEX_CREATE),
    "wfa_hip_seed_index_destroy": (None, [_vp]),
    "wfa_hip_seed_index_query": (_CTYPES, [_vp, _vp] + [_int] * 5 + [_vp] * 6),
    "wfa_hip_seed_index_stats": (_CTYPES, [_vp, _i64p, _i64p, _i64p, _floatp, _floatp]),
    "wfa_hip_seeds_host": (_CTYPES, _SEEDS_HOST),
    "wfa_hip_seed_index_chain": (_CTYPES, [_vp, _vp] + [_int] * 8 + [_vp] * 9),
    "wfa_hip_seed_index_chain_stats": (_CTYPES, [_vp, _floatp, _i64p]),
    "wfa_hip_chains_host": (_CTYPES, _CHAINS_HOST),
    "wfa_hip_seed_index_create_minimizer": (_vp, _INDEX_CREATE),
    "wfa_hip_seed_index_params": (_CTYPES, [_vp] + [_intp] * 3),
    "wfa_hip_minimizers_host": (_CTYPES, [_vp, _i64, _int, _int, _vp, _str, _size]),
    "wfa_hip_seeds_host_minimizer": (_CTYPES, _SEEDS_HOST),
    "wfa_hip_chains_host_minimizer": (_CTYPES, _CHAINS_HOST),
    "wfa_hip_pileup_calls": (_CTYPES, [_vp, _vp, _i32, _i64, _i64, _i32, _vp]),
    "wfa_hip_pileup_sites": (_CTYPES, [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_calls_host": (_CTYPES, [_vp, _vp, _i64, _i32, _vp]),
    "wfa_hip_sites_host": (_CTYPES, [_vp, _vp, _i64, _i32, _i64, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_pileup_track_insertions": (_CTYPES, [_vp, _int]),
    "wfa_hip_pileup_insertion_stats": (_CTYPES, [_vp, _i64p, _i64p]),
    "wfa_hip_pileup_insertions": (_CTYPES, [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _i64, _i64p, _vp, _i64, _i64p, _vp]),
    "wfa_hip_ops_insertions": (_CTYPES, [_vp, _i64, _vp, _i32, _i32, _i64, _i64p, _vp, _i64, _i64p, _vp]),
    "wfa_hip_insertions_host": (_CTYPES, [_vp, _i64, _i32, _i64, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64p, _vp, _i64, _i64p, _vp]),
    "wfa_hip_pileup_track_deletions": (_CTYPES, [_vp, _int]),
    "wfa_hip_pileup_deletion_stats": (_CTYPES, [_vp, _i64p, _i64p]),
    "wfa_hip_pileup_read_deletion_starts": (_CTYPES, [_vp, _i32, _i64, _i64, _vp]),
    "wfa_hip_pileup_deletions": (_CTYPES, [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_ops_deletions": (_CTYPES, [_vp, _i64, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_deletions_host": (_CTYPES, [_vp, _vp, _i64, _i32, _i64, _i32, _i32, _i64, _vp, _vp, _i64, _i64p, _vp]),
    "wfa_hip_pileup_track_strands": (_CTYPES, [_vp, _int]),
    "wfa_hip_pileup_add_strands": (_CTYPES, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "wfa_hip_pileup_read_strand": (_CTYPES, [_vp, _i32, _i64, _i64, _int, _vp]),
    "wfa_hip_pileup_genotypes": (_CTYPES, [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_genotypes_host": (_CTYPES, [_vp, _vp, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_qualset_create": (_vp, [_vp, _vp, _vp, _vp, _vp]),
    "wfa_hip_qualset_destroy": (None, [_vp]),
    "wfa_hip_pileup_track_qualities": (_CTYPES, [_vp, _int]),
    "wfa_hip_pileup_add_quals": (_CTYPES, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "wfa_hip_pileup_read_quality": (_CTYPES, [_vp, _i32, _i64, _i64, _vp]),
    "wfa_hip_pileup_genotypes_quals": (_CTYPES, [_vp, _vp, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_ops_pileup_quals": (_CTYPES, [_vp, _i64, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "wfa_hip_genotypes_quals_host": (_CTYPES, [_vp, _vp, _vp, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _i64, _i64p, _vp]),
    "wfa_hip_batch_left_align": (_CTYPES, [_vp, _vp]),
    "wfa_hip_ops_left_align": (_CTYPES, [_vp, _i64, _vp, _i32, _vp, _i32, _vp]),
    "wfa_hip_batch_sam_counts": (_CTYPES, [_vp, _int, _vp, _i64p, _i64p]),
    "wfa_hip_batch_sam_strings": (_CTYPES, [_vp, _vp, _vp]),
    "wfa_hip_batch_sam_kernel_ms": (_CTYPES, [_vp, _floatp]),
    "wfa_hip_ops_sam": (_CTYPES, [_vp, _i64, _vp, _i32, _i32, _int, _vp, _vp, _i64, _vp, _i64]),
    "wfa_hip_placer_create": (_vp, [_vp, _i64]),
    "wfa_hip_placer_add": (_CTYPES, [_vp] * 6),
    "wfa_hip_placer_add_hits": (_CTYPES, [_vp, _i64] + [_vp] * 7),
    "wfa_hip_placer_run": (_CTYPES, [_vp, _i32, _i32, _vp, _vp]),
    "wfa_hip_placer_count": (_i64, [_vp]),
    "wfa_hip_placer_clear": (_CTYPES, [_vp]),
    "wfa_hip_placer_kernel_ms": (_CTYPES, [_vp, _floatp]),
    "wfa_hip_placer_destroy": (None, [_vp]),
    "wfa_hip_place_host": (_CTYPES, _HITS + [_i32, _i32, _vp, _vp, _str, _size]),
    "wfa_hip_placer_run_pairs": (_CTYPES, [_vp] + [_i32] * 5 + [_i64] + [_vp] * 6),
    "wfa_hip_pair_host": (_CTYPES, _HITS + [_i32] * 5 + [_i64] + [_vp] * 6 + [_str, _size]),
    "wfa_hip_placer_rescue": (_CTYPES, [_vp] * 3 + [_i32] * 5 + [_i64, _vp, _vp] + [_i32] * 3 + [_i64, _i64p, _vp]),
    "wfa_hip_rescue_host": (_CTYPES, _HITS + [_i32] * 5 + [_i64, _vp, _vp, _vp, _i64, _vp] + [_i32] * 3 +
                            [_i64, _i64p, _vp, _str, _size]),
    "wfa_hip_placer_duplicates": (_CTYPES, [_vp] * 2 + [_i32] * 5 + [_i64] + [_vp] * 4),
    "wfa_hip_duplicates_host": (_CTYPES, _HITS + [_i32] * 5 + [_i64, _vp, _vp, _i64, _vp, _vp, _vp, _str, _size]),
    "wfa_hip_placer_add_hits_clips": (_CTYPES, [_vp, _i64] + [_vp] * 9),
    "wfa_hip_placer_read_clips": (_CTYPES, [_vp] * 3),
    "wfa_hip_ops_clips": (_CTYPES, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "wfa_hip_placer_duplicates_ex": (_CTYPES, [_vp] * 2 + [_i32] * 5 + [_i64] + [_vp] * 4 + [_int, _vp, _i32]),
    "wfa_hip_duplicates_host_ex": (_CTYPES, _HITS + [_i32] * 5 + [_i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _int, _vp, _str, _size]),
    "wfa_hip_qsum_host": (_CTYPES, [_vp, _i64, _i32, _vp]),
}
SYMBOLS = list(SIGNATURES)

CROSS_DENSE, CROSS_COMPLETED, CROSS_TOPK = 1, 2, 4
CROSS_MAX_K = 64
SUMMARY_COLS = 10   # M, X, I, D, I runs, D runs, pattern_start, pattern_end, text_start, text_end
SAM_COLS = 8
SAM_COLUMNS = ("pos", "ref_len", "clip_left", "clip_right", "nm", "cigar_len", "md_len", "query_len")
SAM_EQX, SAM_CORE = 1, 2   # WFA_HIP_SAM_EQX: = and X instead of M; WFA_HIP_SAM_CORE: the anchors are M only
PILEUP_COLS = 8
PILEUP_COLUMNS = ("A", "C", "G", "T", "other", "del", "ins", "mismatch")
CALL_CODES = ("A", "C", "G", "T", "other", "del", "no call")   # the low 3 bits of a call byte; CALL_INS: its insertion flag
CALL_NONE, CALL_INS = 6, 8
SITE_COLS = 8
SITE_COLUMNS = ("j", "pos", "ref", "alt", "depth", "ref_count", "alt_count", "ins_count")
INSERTION_COLS = 8
INSERTION_COLUMNS = ("j", "pos", "depth", "ins_count", "allele_count", "allele_len", "alleles", "overflow")
INS_MAX_READS = 4096   # the default of WFA_HIP_INS_MAX_READS
DELETION_COLS = 8
DELETION_COLUMNS = ("j", "pos", "depth", "del_count", "allele_count", "allele_len", "alleles", "overflow")
DEL_MAX_READS = 4096   # the default of WFA_HIP_DEL_MAX_READS
GENOTYPE_COLS = 16
MAX_QUALITY = 93   # WFA_HIP_MAX_QUALITY: raw phred, the printable range of FASTQ
GENOTYPE_COLUMNS = SITE_COLUMNS + ("gt", "gq", "ins_gt", "ins_gq", "depth_fwd", "ref_fwd", "alt_fwd", "ins_fwd")
PLACE_COLS = 8
PLACE_COLUMNS = ("hit", "score", "second", "mapq", "hits", "ties", "text_start", "text_end")
PLACE_NOT_ELIGIBLE, PLACE_OTHER_LOCUS, PLACE_SAME_LOCUS, PLACE_PRIMARY = 0, 1, 2, 3   # the flag byte of a hit
PAIR_COLS = 12
PAIR_COLUMNS = ("hit1", "hit2", "proper", "score", "second", "mapq", "mapq1", "mapq2", "insert", "pairings", "ties", "overflow")
PAIR_MAX_PAIRINGS = 65536
RESCUE_COLS = 8
RESCUE_COLUMNS = ("i", "j", "text_start", "text_len", "reverse", "fragment", "anchor", "spare")
DUP_COLS = 4
DUP_COLUMNS = ("rep", "size", "dup", "overflow")
DUP_MAX_BUCKET = 4096   # WFA_HIP_DUP_MAX_BUCKET
DUP_UNCLIPPED, DUP_BY_QUALITY = 1, 2   # WFA_HIP_DUP_UNCLIPPED: keys on the unclipped ends; WFA_HIP_DUP_BY_QUALITY: scores from base qualities
CLIP_MAX = 65535        # WFA_HIP_CLIP_MAX
INT32_MIN = -2**31
SEED_MAX_N, SEED_MAX_HITS = 16, 4096
SEED_KEYS = ("j", "reverse", "text_start", "text_len", "hits")   # the int32 arrays of a seed query, and overflow (uint8)
CHAIN_MAX_LOOKBACK, CHAIN_MAX_ANCHORS = 64, 65536
MINIMIZER_MAX_W = 32
# the int32 arrays of a chain query, and overflow (uint8)
CHAIN_KEYS = ("j", "reverse", "text_start", "text_len", "hits", "score", "pattern_start", "pattern_len")


def lib():
    """Load libwfa_hip.so (built in-tree by ``__graft_entry__.build()`` / csrc/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} is missing: build it with pywfa_amd/csrc/build.sh "
                          "(there is no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        if restype is not _CTYPES:
            getattr(L, name).restype = restype
        if argtypes is not _CTYPES:
            getattr(L, name).argtypes = argtypes
    if L.wfa_hip_abi_version() != ABI_VERSION:
        raise NativeError("libwfa_hip.so ABI version mismatch: rebuild it")
    _lib = L
    return L


_HOST = False   # False = not looked for yet; None = absent


def compiled_host():
    """pywfa_amd.host._host (Cython, built in-tree by __graft_entry__.build()) bound to the loaded library, or None when the
    extension has not been built (WFA_HIP_NO_COMPILED_HOST=1: ignore it — the ctypes / Python host, for tests)."""
    global _HOST
    if _HOST is False:
        _HOST = None
        if os.environ.get("WFA_HIP_NO_COMPILED_HOST") != "1":
            try:
                from .host import _host
                threads = max(1, min(64, (os.cpu_count() or 2) // 2))
                _host.bind(ctypes.cast(lib().wfa_hip_align_pair, ctypes.c_void_p).value, threads)
                _HOST = _host
            except ImportError:
                _HOST = None
    return _HOST

def default_config():
    c = Config()
    lib().wfa_hip_config_default(ctypes.byref(c))
    return c


def validate(cfg):
    """Return (code, message)."""
    buf = ctypes.create_string_buffer(256)
    rc = lib().wfa_hip_config_validate(ctypes.byref(cfg), buf, 256)
    return rc, buf.value.decode()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ptr_or_null(a):
    """``_ptr`` with NULL for an empty array too."""
    return _ptr(a) if a is not None and a.size else None


def _check_batch(batch):
    if "packed" in batch:
        return _check_packed(batch)
    seqs = np.ascontiguousarray(batch["seqs"], dtype=np.uint8)
    p_off = np.ascontiguousarray(batch["p_off"], dtype=np.int64)
    t_off = np.ascontiguousarray(batch["t_off"], dtype=np.int64)
    p_len = np.ascontiguousarray(batch["p_len"], dtype=np.int32)
    t_len = np.ascontiguousarray(batch["t_len"], dtype=np.int32)
    n = p_len.shape[0]
    if not (p_off.shape[0] == t_off.shape[0] == t_len.shape[0] == n):
        raise ValueError("batch arrays differ in length")
    if n:
        end = lib().wfa_hip_batch_extent(n, _ptr(p_off), _ptr(p_len), _ptr(t_off), _ptr(t_len))   # (host threads: ~1 ms per 10 M pairs)
        if end < 0:
            raise ValueError("negative length or offset")
        if end > seqs.size:
            raise ValueError("sequence offsets run past the blob")
    return seqs, p_off, p_len, t_off, t_len, n


def _check_packed(batch):
    """A batch of 2-bit reads (datagen.to_packed2bits): byte offsets into ``packed``, lengths in bases."""
    packed = np.ascontiguousarray(batch["packed"], dtype=np.uint8)
    p_off = np.ascontiguousarray(batch["p_off"], dtype=np.int64)
    t_off = np.ascontiguousarray(batch["t_off"], dtype=np.int64)
    p_len = np.ascontiguousarray(batch["p_len"], dtype=np.int32)
    t_len = np.ascontiguousarray(batch["t_len"], dtype=np.int32)
    n = p_len.shape[0]
    if not (p_off.shape[0] == t_off.shape[0] == t_len.shape[0] == n):
        raise ValueError("batch arrays differ in length")
    if n:
        end = lib().wfa_hip_batch_extent_packed2bits(n, _ptr(p_off), _ptr(p_len), _ptr(t_off), _ptr(t_len))
        if end < 0:
            raise ValueError("negative length or offset")
        if end > packed.size:
            raise ValueError("sequence offsets run past the blob")
    return packed, p_off, p_len, t_off, t_len, n


def cigar_sprint_pretty(ops, pattern, text):
    """wfa_hip_cigar_sprint_pretty (host only): the text WFA2-lib's cigar_print_pretty prints for this op string."""
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    pattern, text = bytes(pattern), bytes(text)
    fn = lib().wfa_hip_cigar_sprint_pretty
    pb = ctypes.c_char_p(pattern) if pattern else None
    tb = ctypes.c_char_p(text) if text else None
    need = fn(_ptr(ops) if ops.size else None, ops.size, pb, len(pattern), tb, len(text), None, 0)
    if need < 0:
        raise ValueError("wfa_hip_cigar_sprint_pretty: invalid arguments")
    buf = ctypes.create_string_buffer(int(need) + 1)
    fn(_ptr(ops) if ops.size else None, ops.size, pb, len(pattern), tb, len(text), buf, need + 1)
    return buf.value.decode("ascii", "replace")


def _raise_code(rc, what, msg):
    """The exception of a non-OK code of the library."""
    if rc == EINVAL:
        raise ValueError(f"{what}: {msg}")
    if rc == ENOTSUP:
        raise NotImplementedError(f"{what}: {msg}")
    raise NativeError(f"{what}: {msg}")


def _raise_config_refused(cfg, what):
    """The exception of an aligner create that returned NULL: what the validation says of ``cfg``, else the library's global error."""
    msg = lib().wfa_hip_global_error().decode()
    rc, vmsg = validate(cfg)
    if rc == EINVAL:
        raise ValueError(vmsg)
    if rc == ENOTSUP:
        raise NotImplementedError(vmsg)
    raise NativeError(f"{what} failed: {msg}")


class _Checked:
    """``_call``: one call of the library whose non-OK code goes to ``_raise`` under the symbol's name."""

    def _call(self, symbol, *args):
        rc = getattr(lib(), symbol)(*args)
        if rc != OK:
            self._raise(rc, symbol)


class Aligner(_Checked):
    """Owns one wfa_hip_aligner_t (replaces the wavefront_aligner_t* of align.pyx:419)."""

    def __init__(self, cfg, device=0):
        self._pair_caller = None
        self._pair_align = None
        self._h = lib().wfa_hip_create(ctypes.byref(cfg), device)
        if not self._h:
            _raise_config_refused(cfg, "wfa_hip_create")
        self.device = device
        self._batches = weakref.WeakSet()
        self._pair_state = None

    def upload_info(self):
        """wfa_hip_upload_info: what the upload pipeline knows about the host and what its last pipelined upload did."""
        info = np.zeros(8, np.int32)
        if lib().wfa_hip_upload_info(self._h, _ptr(info), 8) != OK:
            raise NativeError("wfa_hip_upload_info failed")
        keys = ("gpu_numa_node", "gpu_node_cpus", "numa_mode", "input_numa_node", "workers_bound", "pack_threads", "copy_threads", "process_cpus")
        return dict(zip(keys, (int(x) for x in info)))

    def close(self):
        if getattr(self, "_h", None):
            # resident batches hold device blocks of this aligner's pool: they go first (the library would also keep
            # the handle alive until the last batch is destroyed)
            for rb in list(self._batches):
                rb.close()
            lib().wfa_hip_destroy(self._h)
            self._h = None
            self._pair_caller = None
            self._pair_align = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self):
        return lib().wfa_hip_last_error(self._h).decode()

    def _raise(self, rc, what):
        _raise_code(rc, what, self.error())

    def set_config(self, cfg):
        self._call("wfa_hip_set_config", self._h, ctypes.byref(cfg))

    def get_config(self):
        c = Config()
        lib().wfa_hip_get_config(self._h, ctypes.byref(c))
        return c

    def align_batch(self, batch, want_cigar, out=None):
        """Host-buffer path (wfa_hip_align_batch). Returns score, status, (ops, begin, len) or None.
        out = (score, status): int32 arrays of the batch size to write into (a loop over equally sized batches then
        touches no fresh pages: zero-filling 2 x 40 MB for 10 M pairs costs about as much as the device work)."""
        seqs, p_off, p_len, t_off, t_len, n = _check_batch(batch)
        if out is not None:
            score, status = out
            if not (score.dtype == np.int32 and status.dtype == np.int32 and score.shape == (n,) and status.shape == (n,)
                    and score.flags.c_contiguous and status.flags.c_contiguous):
                raise ValueError("out: two contiguous int32 arrays of the batch size")
        else:
            score = np.zeros(n, np.int32)
            status = np.zeros(n, np.int32)
        if want_cigar:
            cigar_off = np.zeros(n + 1, np.int64)
            np.cumsum(p_len.astype(np.int64) + t_len.astype(np.int64), out=cigar_off[1:])
            ops = np.zeros(max(int(cigar_off[-1]), 1), np.uint8)
            cbeg = np.zeros(n, np.int64)
            clen = np.zeros(n, np.int32)
        else:
            cigar_off = ops = cbeg = clen = None
        entry = lib().wfa_hip_align_batch_packed2bits if "packed" in batch else lib().wfa_hip_align_batch
        rc = entry(self._h, n, _ptr(seqs), _ptr(p_off), _ptr(p_len), _ptr(t_off),
                   _ptr(t_len), _ptr(score), _ptr(status), _ptr(ops),
                   _ptr(cigar_off), _ptr(cbeg), _ptr(clen))
        if rc != OK:
            self._raise(rc, "wfa_hip_align_batch_packed2bits" if "packed" in batch else "wfa_hip_align_batch")
        return score, status, ((ops, cbeg, clen) if want_cigar else None)

    def align_pair(self, pattern, text, want_cigar):
        """wfa_hip_align_pair: one pair of ASCII ``bytes`` per call, without NumPy arrays on the way (pywfa's loop of
        ``wavefront_align(text)``).  Returns score, status, op bytes (or None).  Through the compiled host
        (pywfa_amd/host/_host.pyx: no ctypes marshalling) when it is built, through ctypes otherwise."""
        pa = self._pair_align   # (the compiled host's bound method, looked up once per aligner: this is pywfa's one-pair-per-call loop)
        if pa is None:
            if not self._h:
                raise NativeError("wfa_hip_align_pair: the aligner is closed")
            host = compiled_host()
            if host is not None:
                self._pair_caller = host.PairCaller(self._h)
                pa = self._pair_align = self._pair_caller.align
        if pa is not None:
            rc, score, status, ops = pa(pattern, text, want_cigar)
            if rc != OK:
                self._raise(rc, "wfa_hip_align_pair")
            return score, status, ops
        st = self._pair_state
        if st is None:
            st = self._pair_state = {"score": ctypes.c_int32(0), "status": ctypes.c_int32(0), "cbeg": ctypes.c_int64(0),
                                     "clen": ctypes.c_int32(0), "ops": None, "cap": 0, "fn": lib().wfa_hip_align_pair}
            st["refs"] = (ctypes.byref(st["score"]), ctypes.byref(st["status"]), ctypes.byref(st["cbeg"]), ctypes.byref(st["clen"]))
        plen, tlen = len(pattern), len(text)
        ops = None
        if want_cigar:
            if st["cap"] < plen + tlen:
                st["cap"] = max(1024, 2 * (plen + tlen))
                st["ops"] = ctypes.create_string_buffer(st["cap"])
            ops = st["ops"]
        r = st["refs"]
        rc = st["fn"](self._h, pattern, plen, text, tlen, r[0], r[1], ops, r[2], r[3])
        if rc != OK:
            self._raise(rc, "wfa_hip_align_pair")
        if not want_cigar:
            return st["score"].value, st["status"].value, None
        b = st["cbeg"].value
        return st["score"].value, st["status"].value, ops.raw[b:b + st["clen"].value]

    def batch(self, batch):
        return ResidentBatch(self, batch)

    def seqset(self, seqs, off, length):
        return SeqSet(self, seqs, off, length)

    def batch_indexed(self, patterns, texts, i, j):
        """wfa_hip_batch_create_indexed: the ResidentBatch whose pair q is (patterns[i[q]], texts[j[q]]) of two SeqSets (texts None:
        both indices into ``patterns``)."""
        return ResidentBatch.indexed(self, patterns, texts, i, j)

    def batch_windows(self, patterns, texts, i, j, p_start=None, p_len=None, t_start=None, t_len=None, reverse=None):
        """wfa_hip_batch_create_windows: the ResidentBatch whose pair q is the window [p_start[q], + p_len[q]) of patterns[i[q]]
        (reverse-complemented where reverse[q]) against the window [t_start[q], + t_len[q]) of texts[j[q]]."""
        return ResidentBatch.windows(self, patterns, texts, i, j, p_start, p_len, t_start, t_len, reverse)

    def pileup(self, texts):
        """wfa_hip_pileup_create: a zeroed Pileup over the bases of a SeqSet."""
        return Pileup(self, texts)

    def qualset(self, reads, quals, off, length):
        """wfa_hip_qualset_create: the base qualities (raw phred) of the sequences of a SeqSet."""
        return QualSet(self, reads, quals, off, length)

    def placer(self, nreads):
        """wfa_hip_placer_create: a Placer over reads 0 .. nreads - 1, without hits."""
        return Placer(self, nreads)

    def seed_index(self, texts, k=13, stride=1, max_occ=64, w=None):
        """wfa_hip_seed_index_create: the k-mer index of a SeqSet (4^k * 4 bytes + 8 bytes per indexed position in HBM).  ``w``:
        wfa_hip_seed_index_create_minimizer instead, the (w,k)-minimizers of the texts (``stride`` plays no part)."""
        return SeedIndex(self, texts, k, stride, max_occ, w)

    def cross(self, patterns, texts=None, want=CROSS_DENSE, k=None):
        """wfa_hip_cross_run of two SeqSets (texts None: all-vs-all of ``patterns``); wfa_hip_cross_run_k when ``k`` is given."""
        return CrossRun(self, patterns, texts, want, k)


def pack_2bit(seq, form=-1):
    """wfa_hip_pack_2bit (host only): the 2-bit words of an ASCII sequence and whether a letter outside ACGT was seen."""
    a = np.frombuffer(bytes(seq), dtype=np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, dtype=np.uint8)
    words = np.zeros(max((len(a) + 15) // 16, 1), np.uint32)
    rc = lib().wfa_hip_pack_2bit(_ptr(a) if len(a) else None, len(a), _ptr(words), form)
    if rc < 0:
        raise ValueError("wfa_hip_pack_2bit: invalid arguments")
    return words[:(len(a) + 15) // 16], bool(rc)


def window_2bit(words, start, len, reverse=False):
    """wfa_hip_window_2bit (host only): the words of the window [start, start + len) of a sequence packed by ``pack_2bit``, re-based
    to bit 0 and reverse-complemented when ``reverse``."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    start, n = int(start), int(len)
    if start >= 0 and n > 0 and start + n > 16 * words.shape[0]:
        raise ValueError("wfa_hip_window_2bit: the window ends behind the words")
    out = np.zeros(max((n + 15) // 16, 1), np.uint32)
    rc = lib().wfa_hip_window_2bit(_ptr(words), start, n, int(bool(reverse)), _ptr(out))
    if rc != OK:
        raise ValueError("wfa_hip_window_2bit: negative start or length")
    return out[:(n + 15) // 16]


def ops_summary(ops, plen, tlen):
    """wfa_hip_ops_summary (host only): the row ``ResidentBatch.summary()`` holds for one pair, from its op string (bytes or a uint8
    array of M / X / I / D) and its lengths: int32[10]."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    out = np.zeros(SUMMARY_COLS, np.int32)
    rc = lib().wfa_hip_ops_summary(_ptr(ops) if ops.size else None, ops.size, int(plen), int(tlen), _ptr(out))
    if rc != OK:
        raise ValueError("wfa_hip_ops_summary: invalid arguments")
    return out


def ops_pileup(ops, pattern, tlen, rows=None):
    """wfa_hip_ops_pileup (host only): one pair's contribution to a pileup, from its op string and its ASCII pattern, added to the
    window-relative ``rows`` (int32, shape (tlen, 8); a fresh zeroed array when None), which is returned."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    pattern = np.frombuffer(bytes(pattern), dtype=np.uint8) if not isinstance(pattern, np.ndarray) else np.ascontiguousarray(pattern, dtype=np.uint8)
    tlen = int(tlen)
    if rows is None:
        rows = np.zeros((max(tlen, 0), PILEUP_COLS), np.int32)
    if not (isinstance(rows, np.ndarray) and rows.dtype == np.int32 and rows.shape == (tlen, PILEUP_COLS) and rows.flags.c_contiguous):
        raise ValueError("rows: a contiguous int32 array of shape (tlen, 8)")
    rc = lib().wfa_hip_ops_pileup(_ptr(ops) if ops.size else None, ops.size, _ptr(pattern) if pattern.size else None, pattern.size, tlen,
                                  _ptr(rows) if rows.size else None)
    if rc != OK:
        raise ValueError("wfa_hip_ops_pileup: invalid arguments (an op string that outruns its pair?)")
    return rows


def ops_pileup_quals(ops, pattern, tlen, quals, min_base_quality=0, quality_cap=40, rows=None, qrows=None):
    """wfa_hip_ops_pileup_quals (host only): one pair's contribution to a pileup that tracks qualities; ``quals``: a raw phred value
    per pattern base, in the window's order.  ``(rows, qrows)``, both int32 of shape (tlen, 8), added to when given."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    pattern = np.frombuffer(bytes(pattern), dtype=np.uint8) if not isinstance(pattern, np.ndarray) else np.ascontiguousarray(pattern, dtype=np.uint8)
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    tlen = int(tlen)
    if quals.shape != pattern.shape:
        raise ValueError("quals: one value per pattern base")
    out = []
    for name, a in (("rows", rows), ("qrows", qrows)):
        if a is None:
            a = np.zeros((max(tlen, 0), PILEUP_COLS), np.int32)
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == (tlen, PILEUP_COLS) and a.flags.c_contiguous):
            raise ValueError(f"{name}: a contiguous int32 array of shape (tlen, 8)")
        out.append(a)
    rc = lib().wfa_hip_ops_pileup_quals(_ptr(ops) if ops.size else None, ops.size, _ptr(pattern) if pattern.size else None, pattern.size, tlen,
                                        _ptr(quals) if quals.size else None, int(min_base_quality), int(quality_cap),
                                        _ptr(out[0]) if out[0].size else None, _ptr(out[1]) if out[1].size else None)
    if rc != OK:
        raise ValueError("wfa_hip_ops_pileup_quals: invalid arguments (an op string that outruns its pair, a quality above 93, "
                         f"min_base_quality = {min_base_quality} outside 0 .. 93 or quality_cap = {quality_cap} outside 1 .. 93?)")
    return out[0], out[1]


def ops_left_align(ops, pattern, text):
    """wfa_hip_ops_left_align (host only): one pair's op string (bytes or a uint8 array of M / X / I / D) left-aligned against its ASCII
    pattern and text: (a new uint8 array, runs moved, merges).  ValueError for an op string that does not consume exactly its pair."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8).copy() if not isinstance(ops, np.ndarray) else np.array(ops, dtype=np.uint8)
    pattern = np.frombuffer(bytes(pattern), dtype=np.uint8) if not isinstance(pattern, np.ndarray) else np.ascontiguousarray(pattern, dtype=np.uint8)
    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
    stats = np.zeros(2, np.int64)
    rc = lib().wfa_hip_ops_left_align(_ptr_or_null(ops), ops.size, _ptr_or_null(pattern), pattern.size, _ptr_or_null(text), text.size, _ptr(stats))
    if rc != OK:
        raise ValueError("wfa_hip_ops_left_align: invalid arguments (an op string that does not consume exactly its pair?)")
    return ops, int(stats[0]), int(stats[1])


def ops_sam(ops, text, plen, flags=0):
    """wfa_hip_ops_sam (host only): the SAM fields of one pair from its op string (bytes or a uint8 array of M / X / I / D), its ASCII
    text and the length of its pattern: (row int32[8] in the columns SAM_COLUMNS, the CIGAR as bytes, the MD string as bytes).
    ValueError for unknown flag bits or an op string that does not consume exactly its pair."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
    row = np.zeros(SAM_COLS, np.int32)
    # a token is at most 11 bytes an op (CIGAR) or 12 (MD), the clips and the last number 11 each
    cigar = np.zeros(11 * ops.size + 22, np.uint8)
    md = np.zeros(12 * ops.size + 11, np.uint8)
    rc = lib().wfa_hip_ops_sam(_ptr_or_null(ops), ops.size, _ptr_or_null(text), text.size, int(plen), int(flags), _ptr(row),
                               _ptr(cigar), cigar.size, _ptr(md), md.size)
    if rc != OK:
        raise ValueError("wfa_hip_ops_sam: invalid arguments (unknown flags, or an op string that does not consume exactly its pair?)")
    return row, cigar[:row[5]].tobytes(), md[:row[6]].tobytes()


def _letters_written(rows, bases_cap):
    """The letters an insertions call wrote for ``rows`` into ``bases_cap`` bytes: those of the rows that fit whole."""
    ends = np.cumsum(rows[:, 5].astype(np.int64)) if len(rows) else np.zeros(0, np.int64)
    fit = ends[ends <= bases_cap]
    return int(fit[-1]) if len(fit) else 0


def ops_insertions(ops, pattern, tlen):
    """wfa_hip_ops_insertions (host only): one pair's insertion records from its op string and its ASCII pattern:
    ``(recs, cols)``, recs int32 of shape (records, 3) = (h, n, offset), cols the records' column bytes (0..4) back to back."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    pattern = np.frombuffer(bytes(pattern), dtype=np.uint8) if not isinstance(pattern, np.ndarray) else np.ascontiguousarray(pattern, dtype=np.uint8)
    head = (_ptr(ops) if ops.size else None, ops.size, _ptr(pattern) if pattern.size else None, pattern.size, int(tlen))
    count, ncols = ctypes.c_int64(0), ctypes.c_int64(0)
    if lib().wfa_hip_ops_insertions(*head, 0, ctypes.byref(count), None, 0, ctypes.byref(ncols), None) != OK:
        raise ValueError("wfa_hip_ops_insertions: invalid arguments (an op string that outruns its pair?)")
    recs = np.zeros((count.value, 3), np.int32)
    cols = np.zeros(ncols.value, np.uint8)
    if count.value:
        lib().wfa_hip_ops_insertions(*head, count.value, ctypes.byref(count), _ptr(recs), ncols.value, ctypes.byref(ncols), _ptr_or_null(cols))
    return recs, cols


def insertions_host(counts, rec_row, rec_n, rec_off, cols, seq=0, start=0, min_depth=1, min_permille=500, cap=None, bases_cap=None):
    """wfa_hip_insertions_host (host only): ``(count, rows, bases_count, bases)`` as ``Pileup.insertions`` gives them, for the rows
    ``counts`` (int32, shape (len, 8)) and the records of those rows (row relative to the first, length, offset into ``cols``)."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if counts.ndim != 2 or counts.shape[1] != PILEUP_COLS:
        raise ValueError("counts: int32 of shape (len, 8)")
    rec_row = np.ascontiguousarray(rec_row, dtype=np.int64)
    rec_n = np.ascontiguousarray(rec_n, dtype=np.int32)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
    cols = np.ascontiguousarray(cols, dtype=np.uint8)
    if not rec_row.shape == rec_n.shape == rec_off.shape or rec_row.ndim != 1:
        raise ValueError("rec_row, rec_n and rec_off: one value per record")
    head = (_ptr_or_null(counts), counts.shape[0], int(seq), int(start), int(min_depth), int(min_permille), rec_row.size,
            _ptr_or_null(rec_row), _ptr_or_null(rec_n), _ptr_or_null(rec_off), _ptr_or_null(cols), cols.size)
    what = f"wfa_hip_insertions_host: invalid arguments (min_depth = {min_depth}, min_permille = {min_permille}, cap = {cap}, bases_cap = {bases_cap})"
    count, nbases = ctypes.c_int64(0), ctypes.c_int64(0)
    if cap is None or bases_cap is None:
        if lib().wfa_hip_insertions_host(*head, 0, ctypes.byref(count), None, 0, ctypes.byref(nbases), None) != OK:
            raise ValueError(what)
        cap = count.value if cap is None else cap
        bases_cap = nbases.value if bases_cap is None else bases_cap
    rows = np.zeros((max(int(cap), 0), INSERTION_COLS), np.int32)
    bases = np.zeros(max(int(bases_cap), 0), np.uint8)
    if lib().wfa_hip_insertions_host(*head, int(cap), ctypes.byref(count), _ptr_or_null(rows), int(bases_cap), ctypes.byref(nbases),
                                     _ptr_or_null(bases)) != OK:
        raise ValueError(what)
    rows = rows[:min(count.value, rows.shape[0])]
    return count.value, rows, nbases.value, bases[:_letters_written(rows, bases.shape[0])]


def ops_deletions(ops, plen, tlen):
    """wfa_hip_ops_deletions (host only): one pair's deletion records from its op string: int32 of shape (records, 2) = (h, n), h
    the window-relative row of the first deleted base."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    head = (_ptr(ops) if ops.size else None, ops.size, int(plen), int(tlen))
    count = ctypes.c_int64(0)
    if lib().wfa_hip_ops_deletions(*head, 0, ctypes.byref(count), None) != OK:
        raise ValueError("wfa_hip_ops_deletions: invalid arguments (an op string that outruns its pair?)")
    recs = np.zeros((count.value, 2), np.int32)
    if count.value:
        lib().wfa_hip_ops_deletions(*head, count.value, ctypes.byref(count), _ptr(recs))
    return recs


def deletions_host(counts, starts, rec_row, rec_n, seq=0, start=0, min_depth=1, min_permille=500, cap=None):
    """wfa_hip_deletions_host (host only): ``(count, rows)`` as ``Pileup.deletions`` gives them, for the rows ``counts`` (int32,
    shape (len, 8)), their ``starts`` (int32, len) and the records that start at those rows (row relative to the first, length)."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    starts = np.ascontiguousarray(starts, dtype=np.int32)
    if counts.ndim != 2 or counts.shape[1] != PILEUP_COLS or starts.shape != (counts.shape[0],):
        raise ValueError("counts: int32 of shape (len, 8); starts: one value per row")
    rec_row = np.ascontiguousarray(rec_row, dtype=np.int64)
    rec_n = np.ascontiguousarray(rec_n, dtype=np.int32)
    if rec_row.shape != rec_n.shape or rec_row.ndim != 1:
        raise ValueError("rec_row and rec_n: one value per record")
    head = (_ptr_or_null(counts), _ptr_or_null(starts), counts.shape[0], int(seq), int(start), int(min_depth), int(min_permille), rec_row.size,
            _ptr_or_null(rec_row), _ptr_or_null(rec_n))
    what = f"wfa_hip_deletions_host: invalid arguments (min_depth = {min_depth}, min_permille = {min_permille}, cap = {cap})"
    count = ctypes.c_int64(0)
    if cap is None:
        if lib().wfa_hip_deletions_host(*head, 0, ctypes.byref(count), None) != OK:
            raise ValueError(what)
        cap = count.value
    rows = np.zeros((max(int(cap), 0), DELETION_COLS), np.int32)
    if lib().wfa_hip_deletions_host(*head, int(cap), ctypes.byref(count), _ptr_or_null(rows)) != OK:
        raise ValueError(what)
    return count.value, rows[:min(count.value, rows.shape[0])]


def _calls_rows(counts, ref):
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    ref = np.frombuffer(bytes(ref), dtype=np.uint8) if not isinstance(ref, np.ndarray) else np.ascontiguousarray(ref, dtype=np.uint8)
    if counts.ndim != 2 or counts.shape[1] != PILEUP_COLS or ref.shape != (counts.shape[0],):
        raise ValueError("counts: int32 of shape (len, 8); ref: one byte per row")
    return counts, ref


def calls_host(counts, ref, min_depth=1):
    """wfa_hip_calls_host (host only): the call bytes ``Pileup.calls`` gives for the rows ``counts`` (int32, shape (len, 8), as
    ``Pileup.read`` returns them) over the reference bytes ``ref``: uint8[len]."""
    counts, ref = _calls_rows(counts, ref)
    out = np.zeros(counts.shape[0], np.uint8)
    rc = lib().wfa_hip_calls_host(_ptr(counts) if counts.size else None, _ptr(ref) if ref.size else None, counts.shape[0], int(min_depth),
                                  _ptr(out) if out.size else None)
    if rc != OK:
        raise ValueError(f"wfa_hip_calls_host: invalid arguments (min_depth = {min_depth})")
    return out


def sites_host(counts, ref, seq=0, start=0, min_depth=1, min_permille=500, cap=None):
    """wfa_hip_sites_host (host only): ``(count, rows)`` of the sites among the rows ``counts`` over the reference bytes ``ref``, numbered
    j = seq, pos = start + row; rows: int32 of shape (min(count, cap), 8), every site when ``cap`` is None (a counting call first)."""
    counts, ref = _calls_rows(counts, ref)
    n = counts.shape[0]
    args = (_ptr(counts) if counts.size else None, _ptr(ref) if ref.size else None, n, int(seq), int(start), int(min_depth), int(min_permille))
    count = ctypes.c_int64(0)
    if cap is None:
        if lib().wfa_hip_sites_host(*args, 0, ctypes.byref(count), None) != OK:
            raise ValueError(f"wfa_hip_sites_host: invalid arguments (min_depth = {min_depth}, min_permille = {min_permille})")
        cap = count.value
    rows = np.zeros((max(int(cap), 0), SITE_COLS), np.int32)
    if lib().wfa_hip_sites_host(*args, int(cap), ctypes.byref(count), _ptr(rows) if rows.size else None) != OK:
        raise ValueError(f"wfa_hip_sites_host: invalid arguments (min_depth = {min_depth}, min_permille = {min_permille}, cap = {cap})")
    return count.value, rows[:min(count.value, rows.shape[0])]


def genotypes_host(counts, ref, counts_fwd=None, seq=0, start=0, min_depth=1, min_permille=500, err_q=20, min_alt_strand=0, cap=None):
    """wfa_hip_genotypes_host (host only): ``(count, rows)`` of the genotyped sites among the rows ``counts`` over the reference bytes
    ``ref``; ``counts_fwd``: the forward rows of a pileup that tracks strands (``Pileup.read(strand=0)``), None: not tracking (the
    last four columns are -1).  Rows: int32 of shape (min(count, cap), 16), every one when ``cap`` is None (a counting call first)."""
    counts, ref = _calls_rows(counts, ref)
    if counts_fwd is not None:
        counts_fwd = np.ascontiguousarray(counts_fwd, dtype=np.int32)
        if counts_fwd.shape != counts.shape:
            raise ValueError("counts_fwd: int32 of the shape of counts")
        if not counts_fwd.size:
            counts_fwd = np.zeros((1, PILEUP_COLS), np.int32)   # (tracking is told from a non-NULL pointer, even over no rows)
    n = counts.shape[0]
    args = (_ptr(counts) if counts.size else None, None if counts_fwd is None else _ptr(counts_fwd),
            _ptr(ref) if ref.size else None, n, int(seq), int(start), int(min_depth), int(min_permille), int(err_q), int(min_alt_strand))
    what = (f"wfa_hip_genotypes_host: invalid arguments (min_depth = {min_depth}, min_permille = {min_permille}, err_q = {err_q}, "
            f"min_alt_strand = {min_alt_strand}, cap = {cap})")
    count = ctypes.c_int64(0)
    if cap is None:
        if lib().wfa_hip_genotypes_host(*args, 0, ctypes.byref(count), None) != OK:
            raise ValueError(what)
        cap = count.value
    rows = np.zeros((max(int(cap), 0), GENOTYPE_COLS), np.int32)
    if lib().wfa_hip_genotypes_host(*args, int(cap), ctypes.byref(count), _ptr(rows) if rows.size else None) != OK:
        raise ValueError(what)
    return count.value, rows[:min(count.value, rows.shape[0])]


def genotypes_quals_host(counts, qsums, ref, counts_fwd=None, seq=0, start=0, min_depth=1, min_permille=500, err_q=20, min_alt_strand=0,
                         cap=None):
    """wfa_hip_genotypes_quals_host (host only): ``genotypes_host`` with the costs of "base qualities"; ``qsums``: the rows of the
    quality table (``Pileup.read_quality``), int32 of the shape of ``counts``."""
    counts, ref = _calls_rows(counts, ref)
    qsums = np.ascontiguousarray(qsums, dtype=np.int32)
    if qsums.shape != counts.shape:
        raise ValueError("qsums: int32 of the shape of counts")
    if counts_fwd is not None:
        counts_fwd = np.ascontiguousarray(counts_fwd, dtype=np.int32)
        if counts_fwd.shape != counts.shape:
            raise ValueError("counts_fwd: int32 of the shape of counts")
        if not counts_fwd.size:
            counts_fwd = np.zeros((1, PILEUP_COLS), np.int32)   # (tracking is told from a non-NULL pointer, even over no rows)
    n = counts.shape[0]
    args = (_ptr(counts) if counts.size else None, _ptr(qsums) if qsums.size else None, None if counts_fwd is None else _ptr(counts_fwd),
            _ptr(ref) if ref.size else None, n, int(seq), int(start), int(min_depth), int(min_permille), int(err_q), int(min_alt_strand))
    what = (f"wfa_hip_genotypes_quals_host: invalid arguments (min_depth = {min_depth}, min_permille = {min_permille}, err_q = {err_q}, "
            f"min_alt_strand = {min_alt_strand}, cap = {cap})")
    count = ctypes.c_int64(0)
    if cap is None:
        if lib().wfa_hip_genotypes_quals_host(*args, 0, ctypes.byref(count), None) != OK:
            raise ValueError(what)
        cap = count.value
    rows = np.zeros((max(int(cap), 0), GENOTYPE_COLS), np.int32)
    if lib().wfa_hip_genotypes_quals_host(*args, int(cap), ctypes.byref(count), _ptr(rows) if rows.size else None) != OK:
        raise ValueError(what)
    return count.value, rows[:min(count.value, rows.shape[0])]


def _hit_arrays(i, j, reverse, score, status, text_start, text_end):
    """The arrays of a hit list as the C entries take them: int32 each, ``reverse`` uint8 0 / 1 or None; one length."""
    a = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in
         (("i", i), ("j", j), ("score", score), ("status", status), ("text_start", text_start), ("text_end", text_end))}
    a["reverse"] = None if reverse is None else np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
    n = a["i"].shape[0]
    for k, v in a.items():
        if v is not None and v.shape != (n,):
            raise ValueError(f"{k}: one value per hit ({n})")
    return a, n


def place_host(nreads, i, j, reverse, score, status, text_start, text_end, min_score=INT32_MIN, full_gap=1):
    """wfa_hip_place_host (host only): ``(rows, flags)`` of the placement rule over a list of hits in hit-number order — rows int32 of
    shape (nreads, 8) in the columns PLACE_COLUMNS, flags uint8 per hit; what ``Placer.add_hits`` + ``Placer.run`` give."""
    a, n = _hit_arrays(i, j, reverse, score, status, text_start, text_end)
    nreads = int(nreads)
    rows = np.zeros((max(nreads, 0), PLACE_COLS), np.int32)
    flags = np.zeros(n, np.uint8)
    msg = ctypes.create_string_buffer(256)
    p = _ptr_or_null
    rc = lib().wfa_hip_place_host(nreads, n, p(a["i"]), p(a["j"]), p(a["reverse"]), p(a["score"]), p(a["status"]), p(a["text_start"]),
                                  p(a["text_end"]), int(min_score), int(full_gap), p(rows), p(flags), msg, 256)
    if rc != OK:
        raise ValueError(f"wfa_hip_place_host: {msg.value.decode()}")
    return rows, flags


def _mate_arrays(mates):
    """``(nfrag, mate1, mate2)`` of the ``mates`` argument of the pairing entries: an int (that many interleaved fragments, no arrays)
    or an (F, 2) integer array of read indices (two contiguous int32 columns)."""
    if isinstance(mates, (int, np.integer)) and not isinstance(mates, bool):
        return int(mates), None, None
    m = np.asarray(mates)
    if m.ndim != 2 or m.shape[1] != 2 or (m.size and not np.issubdtype(m.dtype, np.integer)):
        raise ValueError(f"mates: an integer array of shape (F, 2) or a number of interleaved fragments, got shape {m.shape} of {m.dtype}")
    if m.size and (m.min() < -2**31 or m.max() >= 2**31):
        raise ValueError("mates: an index does not fit 32 bits")
    return m.shape[0], np.ascontiguousarray(m[:, 0], dtype=np.int32), np.ascontiguousarray(m[:, 1], dtype=np.int32)


def _mate_ptrs(mates):
    """``(nfrag, mate1, mate2)`` as the C entries take them: ``_mate_arrays`` as pointers (which keep their arrays alive), NULL for
    interleaved mates only: an empty mate array is still "given"."""
    nfrag, m1, m2 = _mate_arrays(mates)
    return nfrag, _ptr(m1), _ptr(m2)


def pair_host(nreads, i, j, reverse, score, status, text_start, text_end, mates, min_score=INT32_MIN, full_gap=1, min_insert=0,
              max_insert=1000, unpaired=0):
    """wfa_hip_pair_host (host only): ``(rows, flags, pair_rows, pair_flags)`` of the pairing rule over a list of hits in hit-number
    order — rows and flags as ``place_host`` gives them, pair_rows int32 of shape (F, 12) in the columns PAIR_COLUMNS, pair_flags uint8
    per hit; what ``Placer.add_hits`` + ``Placer.run_pairs`` give.  ``mates``: an (F, 2) integer array of read indices, or an int F:
    interleaved, fragment f being reads 2 f and 2 f + 1."""
    a, n = _hit_arrays(i, j, reverse, score, status, text_start, text_end)
    nfrag, m1, m2 = _mate_ptrs(mates)
    nreads = int(nreads)
    rows = np.zeros((max(nreads, 0), PLACE_COLS), np.int32)
    flags = np.zeros(n, np.uint8)
    pair_rows = np.zeros((max(nfrag, 0), PAIR_COLS), np.int32)
    pair_flags = np.zeros(n, np.uint8)
    msg = ctypes.create_string_buffer(256)
    p = _ptr_or_null
    rc = lib().wfa_hip_pair_host(nreads, n, p(a["i"]), p(a["j"]), p(a["reverse"]), p(a["score"]), p(a["status"]), p(a["text_start"]),
                                 p(a["text_end"]), int(min_score), int(full_gap), int(min_insert), int(max_insert), int(unpaired), nfrag,
                                 m1, m2, p(rows), p(flags), p(pair_rows), p(pair_flags), msg, 256)
    if rc != OK:
        raise ValueError(f"wfa_hip_pair_host: {msg.value.decode()}")
    return rows, flags, pair_rows, pair_flags


def rescue_host(nreads, i, j, reverse, score, status, text_start, text_end, mates, read_len, text_len, min_score=INT32_MIN, full_gap=1,
                min_insert=0, max_insert=1000, unpaired=0, pad=16, min_len=0, anchor_mapq=0, cap=None):
    """wfa_hip_rescue_host (host only): ``(count, rows)`` of the rescue rule over a list of hits in hit-number order, the reads' lengths
    ``read_len`` (one per read) and the texts' lengths ``text_len`` — rows int32 of shape (min(count, cap), 8) in the columns
    RESCUE_COLUMNS, every window when ``cap`` is None (a counting call first); what ``Placer.add_hits`` + ``Placer.rescue`` give."""
    a, n = _hit_arrays(i, j, reverse, score, status, text_start, text_end)
    nfrag, m1, m2 = _mate_ptrs(mates)
    nreads = int(nreads)
    read_len = np.ascontiguousarray(read_len, dtype=np.int32)
    text_len = np.ascontiguousarray(text_len, dtype=np.int32)
    if read_len.shape != (max(nreads, 0),):
        raise ValueError(f"read_len: one value per read ({nreads})")
    if text_len.ndim != 1:
        raise ValueError("text_len: one value per text")
    msg = ctypes.create_string_buffer(256)
    p = _ptr_or_null
    args = (nreads, n, p(a["i"]), p(a["j"]), p(a["reverse"]), p(a["score"]), p(a["status"]), p(a["text_start"]), p(a["text_end"]),
            int(min_score), int(full_gap), int(min_insert), int(max_insert), int(unpaired), nfrag, m1, m2, p(read_len),
            text_len.shape[0], p(text_len), int(pad), int(min_len), int(anchor_mapq))
    count = ctypes.c_int64(0)
    if cap is None:
        if lib().wfa_hip_rescue_host(*args, 0, ctypes.byref(count), None, msg, 256) != OK:
            raise ValueError(f"wfa_hip_rescue_host: {msg.value.decode()}")
        cap = count.value
    rows = np.zeros((max(int(cap), 0), RESCUE_COLS), np.int32)
    if lib().wfa_hip_rescue_host(*args, int(cap), ctypes.byref(count), p(rows), msg, 256) != OK:
        raise ValueError(f"wfa_hip_rescue_host: {msg.value.decode()}")
    return count.value, rows[:min(count.value, rows.shape[0])]


def _clip_arrays(lead, trail, n):
    """``lead`` and ``trail`` of n hits as the C entries take them: int32 each, or None."""
    out = []
    for name, c in (("lead", lead), ("trail", trail)):
        c = None if c is None else np.ascontiguousarray(c, dtype=np.int32)
        if c is not None and c.shape != (n,):
            raise ValueError(f"{name}: one value per hit ({n})")
        out.append(c)
    return out


def ops_clips(ops, plen, tlen):
    """wfa_hip_ops_clips (host only): ``(lead, trail)`` of one pair, the pattern bases (X and D ops) in front of the first and behind
    the last M of its op string, each saturated at CLIP_MAX; (0, 0) without an M or for an empty pair."""
    ops = np.frombuffer(bytes(ops), dtype=np.uint8) if not isinstance(ops, np.ndarray) else np.ascontiguousarray(ops, dtype=np.uint8)
    lead, trail = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib().wfa_hip_ops_clips(_ptr(ops) if ops.size else None, ops.size, int(plen), int(tlen), ctypes.byref(lead), ctypes.byref(trail))
    if rc != OK:
        raise ValueError("wfa_hip_ops_clips: invalid arguments")
    return lead.value, trail.value


def qsum_host(quals, min_quality=15):
    """wfa_hip_qsum_host (host only): the sum of the raw phred values of one read (a uint8 array) that are at least ``min_quality``
    (0 .. 93), saturated to 2^31 - 1."""
    quals = np.ascontiguousarray(quals, dtype=np.uint8)
    out = ctypes.c_int32(0)
    if quals.ndim != 1 or lib().wfa_hip_qsum_host(_ptr(quals) if quals.size else None, quals.size, int(min_quality), ctypes.byref(out)) != OK:
        raise ValueError(f"wfa_hip_qsum_host: invalid arguments (min_quality = {min_quality}: 0 .. {MAX_QUALITY})")
    return out.value


def duplicates_host(nreads, i, j, reverse, score, status, text_start, text_end, mates, text_len, min_score=INT32_MIN, full_gap=1,
                    min_insert=0, max_insert=1000, unpaired=0, lead=None, trail=None, flags=None, qsum=None):
    """wfa_hip_duplicates_host (host only): ``(read_rows, pair_rows)`` of the duplicate rule over a list of hits in hit-number order and
    the texts' lengths ``text_len`` — int32 of shape (nreads, 4) and (F, 4) in the columns DUP_COLUMNS; what ``Placer.add_hits`` +
    ``Placer.duplicates`` give.  ``mates`` as for ``pair_host``; 0: the single-end form.  With any of ``lead`` / ``trail`` (the clips
    per hit), ``flags`` (DUP_UNCLIPPED | DUP_BY_QUALITY) or ``qsum`` (int32 per read, for DUP_BY_QUALITY):
    wfa_hip_duplicates_host_ex."""
    a, n = _hit_arrays(i, j, reverse, score, status, text_start, text_end)
    ex = not (lead is None and trail is None and flags is None and qsum is None)
    lead, trail = _clip_arrays(lead, trail, n)
    if qsum is not None:
        qsum = np.ascontiguousarray(qsum, dtype=np.int32)
        if qsum.shape != (max(int(nreads), 0),):
            raise ValueError(f"qsum: one value per read ({nreads})")
    nfrag, m1, m2 = _mate_ptrs(mates)
    nreads = int(nreads)
    text_len = np.ascontiguousarray(text_len, dtype=np.int32)
    if text_len.ndim != 1:
        raise ValueError("text_len: one value per text")
    read_rows = np.zeros((max(nreads, 0), DUP_COLS), np.int32)
    pair_rows = np.zeros((max(nfrag, 0), DUP_COLS), np.int32)
    msg = ctypes.create_string_buffer(256)
    p = _ptr_or_null
    head = (nreads, n, p(a["i"]), p(a["j"]), p(a["reverse"]), p(a["score"]), p(a["status"]), p(a["text_start"]), p(a["text_end"]),
            int(min_score), int(full_gap), int(min_insert), int(max_insert), int(unpaired), nfrag, m1, m2, text_len.shape[0], p(text_len),
            p(read_rows), p(pair_rows))
    if ex:   # (qsum: _ptr, so that an empty array is still "given")
        rc = lib().wfa_hip_duplicates_host_ex(*head, p(lead), p(trail), int(flags or 0), _ptr(qsum), msg, 256)
    else:
        rc = lib().wfa_hip_duplicates_host(*head, msg, 256)
    if rc != OK:
        raise ValueError(f"wfa_hip_duplicates_host{'_ex' if ex else ''}: {msg.value.decode()}")
    return read_rows, pair_rows


def seeds_host(read, texts, k=13, stride=1, max_occ=64, n=4, min_hits=2, gap=16, pad=16, max_hits=2048, w=None):
    """wfa_hip_seeds_host (host only): the row ``SeedIndex.query`` holds for ONE read (bytes) against the texts (a list of bytes, or a
    blob dict(seqs=, off=, len=) made once for many reads): dict of int32[n] ``j`` / ``reverse`` / ``text_start`` / ``text_len`` /
    ``hits`` and ``overflow`` (0 or 1).  ``w``: wfa_hip_seeds_host_minimizer, the row under a minimizer index (``stride`` plays no
    part).  ValueError (naming the parameter) for a parameter out of range."""
    read = np.frombuffer(bytes(read), dtype=np.uint8) if not isinstance(read, np.ndarray) else np.ascontiguousarray(read, dtype=np.uint8)
    if not isinstance(texts, dict):
        texts = seeds_host_texts(texts)
    rows = max(int(n), 1) if isinstance(n, (int, np.integer)) else 1
    out = {key: np.zeros(rows, np.int32) for key in SEED_KEYS}
    over = np.zeros(1, np.uint8)
    msg = ctypes.create_string_buffer(256)
    entry = lib().wfa_hip_seeds_host if w is None else lib().wfa_hip_seeds_host_minimizer
    rc = entry(_ptr(read) if read.size else None, read.size, texts["len"].shape[0], _ptr(texts["seqs"]), _ptr(texts["off"]),
               _ptr(texts["len"]), k, stride if w is None else w, max_occ, n, min_hits, gap, pad, max_hits,
               *[_ptr(out[key]) for key in SEED_KEYS], _ptr(over), msg, len(msg))
    if rc != OK:
        raise ValueError(f"{'wfa_hip_seeds_host' if w is None else 'wfa_hip_seeds_host_minimizer'}: {msg.value.decode()}")
    out["overflow"] = int(over[0])
    return out


def chains_host(read, texts, k=13, stride=1, max_occ=64, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64,
                max_anchors=16384, w=None):
    """wfa_hip_chains_host (host only): the row ``SeedIndex.chain`` holds for ONE read (bytes) against the texts (a list of bytes, or
    the blob of ``seeds_host_texts``): dict of int32[n] per key of ``CHAIN_KEYS`` and ``overflow`` (0 or 1).  ``w``:
    wfa_hip_chains_host_minimizer, the row under a minimizer index (``stride`` plays no part).  ValueError (naming the parameter) for
    a parameter out of range."""
    read = np.frombuffer(bytes(read), dtype=np.uint8) if not isinstance(read, np.ndarray) else np.ascontiguousarray(read, dtype=np.uint8)
    if not isinstance(texts, dict):
        texts = seeds_host_texts(texts)
    rows = max(int(n), 1) if isinstance(n, (int, np.integer)) else 1
    out = {key: np.zeros(rows, np.int32) for key in CHAIN_KEYS}
    over = np.zeros(1, np.uint8)
    msg = ctypes.create_string_buffer(256)
    entry = lib().wfa_hip_chains_host if w is None else lib().wfa_hip_chains_host_minimizer
    rc = entry(_ptr(read) if read.size else None, read.size, texts["len"].shape[0], _ptr(texts["seqs"]), _ptr(texts["off"]),
               _ptr(texts["len"]), k, stride if w is None else w, max_occ, n, min_hits, min_score, lookback, max_dist, band, pad,
               max_anchors, *[_ptr(out[key]) for key in CHAIN_KEYS], _ptr(over), msg, len(msg))
    if rc != OK:
        raise ValueError(f"{'wfa_hip_chains_host' if w is None else 'wfa_hip_chains_host_minimizer'}: {msg.value.decode()}")
    out["overflow"] = int(over[0])
    return out


def minimizers_host(seq, k, w):
    """wfa_hip_minimizers_host (host only): bool[len(seq)], True at the (w,k)-minimizers of ONE sequence (bytes).  ValueError (naming
    the parameter) for ``k`` or ``w`` out of range."""
    seq = np.frombuffer(bytes(seq), dtype=np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, dtype=np.uint8)
    flags = np.zeros(seq.size, np.uint8)
    msg = ctypes.create_string_buffer(256)
    rc = lib().wfa_hip_minimizers_host(_ptr(seq) if seq.size else None, seq.size, k, w, _ptr(flags) if seq.size else None, msg, len(msg))
    if rc != OK:
        raise ValueError(f"wfa_hip_minimizers_host: {msg.value.decode()}")
    return flags.astype(bool)


def seeds_host_texts(texts):
    """The text set of ``seeds_host`` as one blob: dict(seqs= uint8, off= int64, len= int32)."""
    texts = [bytes(t) for t in texts]
    length = np.fromiter((len(t) for t in texts), np.int32, len(texts))
    off = np.zeros(len(texts), np.int64)
    if len(texts) > 1:
        off[1:] = np.cumsum(length[:-1], dtype=np.int64)
    seqs = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8)
    return dict(seqs=seqs, off=off, len=length)


def plan_host_threads(sharers, hw_threads=None):
    """wfa_hip_plan_host_threads: (pack, copy) threads of ONE device's upload pipeline when `sharers` aligners / processes feed GPUs
    from this host (host only)."""
    pack, copy = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().wfa_hip_plan_host_threads(int(sharers), int(hw_threads or os.cpu_count() or 1), ctypes.byref(pack), ctypes.byref(copy))
    if rc != OK:
        raise ValueError("wfa_hip_plan_host_threads: invalid arguments")
    return pack.value, copy.value


def plan_shards(p_len, t_len, nshards):
    """wfa_hip_plan_shards: contiguous shards balanced by sum(p_len + t_len). Returns int64[nshards + 1] (host only)."""
    p_len = np.ascontiguousarray(p_len, dtype=np.int32)
    t_len = np.ascontiguousarray(t_len, dtype=np.int32)
    out = np.zeros(nshards + 1, np.int64)
    rc = lib().wfa_hip_plan_shards(len(p_len), _ptr(p_len), _ptr(t_len), nshards, _ptr(out))
    if rc != OK:
        raise ValueError("wfa_hip_plan_shards: invalid arguments")
    return out


def plan_cross_bands(m, n, triangle, max_pairs):
    """wfa_hip_plan_cross_bands: the first row of every band of a cross run and the end, int64[nbands + 1] (host only)."""
    nb = lib().wfa_hip_plan_cross_bands(int(m), int(n), int(bool(triangle)), int(max_pairs), None, 0)
    if nb < 0:
        raise ValueError("wfa_hip_plan_cross_bands: invalid arguments")
    out = np.zeros(nb + 1, np.int64)
    lib().wfa_hip_plan_cross_bands(int(m), int(n), int(bool(triangle)), int(max_pairs), _ptr(out), nb + 1)
    return out


class _Handle(_Checked):
    """What the resident handles share: the ``aligner`` they belong to (its ``close()`` closes them first), the native handle ``_h``,
    and an idempotent ``close()`` through the destroy symbol the class names."""

    _destroy = None              # the symbol that frees _h
    _device_failure = "failed"   # a refused create whose message holds this is a NativeError, any other a ValueError
    aligner = None
    _h = None                    # (also of an object whose constructor raised: close() and __del__ then do nothing)

    def _created(self, handle, what, refused=ValueError):
        """Keep the handle a create returned and register with the aligner, or raise its last error under the symbol's name."""
        self._h = handle
        if not handle:
            msg = self.aligner.error()
            raise (NativeError if self._device_failure in msg else refused)(f"{what}: {msg}")
        self.aligner._batches.add(self)

    def _raise(self, rc, what):
        self.aligner._raise(rc, what)

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeqSet(_Handle):
    """A set of sequences resident in HBM, 2-bit packed once (wfa_hip_seqset_t).  ``seqs`` / ``off`` / ``len`` as a batch's blob:
    sequence k = seqs[off[k] .. +len[k])."""

    _destroy = "wfa_hip_seqset_destroy"

    def __init__(self, aligner, seqs, off, length):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int32)
        n = length.shape[0]
        if off.shape[0] != n:
            raise ValueError("sequence set arrays differ in length")
        if n and (int(off.min()) < 0 or int(length.min()) < 0):
            raise ValueError("negative length or offset")
        if n and int((off + length).max()) > seqs.size:
            raise ValueError("sequence offsets run past the blob")
        self.aligner = aligner
        self.n = n
        self.length = length.copy()   # (an indexed batch sizes its op buffers from the lengths)
        self._created(lib().wfa_hip_seqset_create(aligner._h, n, _ptr(seqs) if seqs.size else None, _ptr(off), _ptr(length)),
                      "wfa_hip_seqset_create")


class QualSet(_Handle):
    """The base qualities of the sequences of a SeqSet, resident in HBM (wfa_hip_qualset_t): a byte per base, raw phred 0 .. 93;
    entry k = quals[off[k] .. +len[k]), len[k] the length of sequence k of ``reads``.  Stays valid after ``reads`` is closed."""

    _destroy = "wfa_hip_qualset_destroy"

    def __init__(self, aligner, reads, quals, off, length):
        if not reads._h:
            raise ValueError("the sequence set is closed")
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int32)
        n = length.shape[0]
        if off.shape[0] != n or n != reads.n:
            raise ValueError(f"quality set: one entry per sequence of the set ({reads.n})")
        if n and (int(off.min()) < 0 or int(length.min()) < 0):
            raise ValueError("negative length or offset")
        if n and int((off + length).max()) > quals.size:
            raise ValueError("quality offsets run past the blob")
        self.aligner = aligner
        self.n = n
        self.length = length.copy()
        self._created(lib().wfa_hip_qualset_create(aligner._h, reads._h, _ptr(quals) if quals.size else None, _ptr(off), _ptr(length)),
                      "wfa_hip_qualset_create")


class CrossRun(_Handle):
    """The results of one cross run, resident in HBM (wfa_hip_cross_t)."""

    _destroy = "wfa_hip_cross_destroy"

    def __init__(self, aligner, patterns, texts=None, want=CROSS_DENSE, k=None):
        self.aligner = aligner
        self.m = patterns.n
        self.n = patterns.n if texts is None else texts.n
        self.k = 0 if k is None else int(k)
        th = None if texts is None else texts._h
        if k is None:
            h = lib().wfa_hip_cross_run(aligner._h, patterns._h, th, int(want))
        else:
            h = lib().wfa_hip_cross_run_k(aligner._h, patterns._h, th, int(want), self.k)
        self._created(h, "wfa_hip_cross_run")

    def dense(self):
        score = np.zeros((self.m, self.n), np.int32)
        status = np.zeros((self.m, self.n), np.int32)
        self._call("wfa_hip_cross_dense", self._h, _ptr(score), _ptr(status))
        return score, status

    def completed(self):
        count = ctypes.c_int64(0)
        self._call("wfa_hip_cross_completed", self._h, ctypes.byref(count), None, None, None)
        out = {k: np.zeros(count.value, np.int32) for k in ("i", "j", "score")}
        if count.value:
            self._call("wfa_hip_cross_completed", self._h, ctypes.byref(count), _ptr(out["i"]), _ptr(out["j"]), _ptr(out["score"]))
        return out

    def topk(self):
        """wfa_hip_cross_topk: dict(j=, score=), int32 arrays of shape (m, k)."""
        out = {key: np.zeros((self.m, self.k), np.int32) for key in ("j", "score")}
        self._call("wfa_hip_cross_topk", self._h, _ptr(out["j"]), _ptr(out["score"]))
        return out

    def kernel_ms(self):
        ms = ctypes.c_float(0)
        pairs = ctypes.c_int64(0)
        self._call("wfa_hip_cross_kernel_ms", self._h, ctypes.byref(ms), ctypes.byref(pairs))
        return ms.value, pairs.value


class Pileup(_Handle):
    """Per-base counters over a text SeqSet, resident in HBM (wfa_hip_pileup_t): 32 bytes per text base, int32 counters without an
    overflow check.  Stays valid after the set is closed.  ``tracking``: whether it keeps the insertion log (``track_insertions``);
    ``deletions_tracked``: whether it keeps the deletion log and the starts plane (``track_deletions``: 4 more bytes per text base);
    ``strands``: whether it keeps the forward table (``track_strands``: 32 more bytes per text base); ``qualities``: whether it keeps
    the quality table (``track_qualities``: 32 more bytes per text base)."""

    _destroy = "wfa_hip_pileup_destroy"
    tracking = False
    deletions_tracked = False
    strands = False
    qualities = False

    def __init__(self, aligner, texts):
        if not texts._h:
            raise ValueError("sequence set is closed")
        self.aligner = aligner
        self.n = texts.n
        self.length = texts.length
        self._created(lib().wfa_hip_pileup_create(aligner._h, texts._h), "wfa_hip_pileup_create")

    def add(self, batch, j, t_start=None, keep=None, reverse=None):
        """wfa_hip_pileup_add: the pairs of a ResidentBatch after its full-scope run, pair q against texts[j[q]] from t_start[q].  On a
        pileup that tracks strands, wfa_hip_pileup_add_strands: ``reverse[q]`` != 0 is a reverse pair, None: every pair is forward
        (a ``reverse`` on a pileup that does not track goes to that call too, which refuses it)."""
        j = np.ascontiguousarray(j, dtype=np.int32)
        t_start = None if t_start is None else np.ascontiguousarray(t_start, dtype=np.int32)
        keep = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        reverse = None if reverse is None else np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
        for name, a in (("j", j), ("t_start", t_start), ("keep", keep), ("reverse", reverse)):
            if a is not None and a.shape != (batch.n,):
                raise ValueError(f"{name}: one value per pair of the batch ({batch.n})")
        if self.strands or reverse is not None:
            self._call("wfa_hip_pileup_add_strands", self._h, batch._h, _ptr(j), _ptr(t_start), _ptr(keep), _ptr(reverse))
        else:
            self._call("wfa_hip_pileup_add", self._h, batch._h, _ptr(j), _ptr(t_start), _ptr(keep))

    def add_quals(self, batch, j, quals, i, t_start=None, keep=None, reverse=None, p_start=None, min_base_quality=0, quality_cap=40):
        """wfa_hip_pileup_add_quals: ``add`` on a pileup that tracks qualities (with or without strands): pair q is the window from
        ``p_start[q]`` of read ``i[q]`` of the QualSet ``quals``, reversed where ``reverse[q]``."""
        j = np.ascontiguousarray(j, dtype=np.int32)
        i = np.ascontiguousarray(i, dtype=np.int32)
        t_start = None if t_start is None else np.ascontiguousarray(t_start, dtype=np.int32)
        p_start = None if p_start is None else np.ascontiguousarray(p_start, dtype=np.int32)
        keep = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        reverse = None if reverse is None else np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
        for name, a in (("j", j), ("i", i), ("t_start", t_start), ("p_start", p_start), ("keep", keep), ("reverse", reverse)):
            if a is not None and a.shape != (batch.n,):
                raise ValueError(f"{name}: one value per pair of the batch ({batch.n})")
        if not quals._h:
            raise ValueError("the quality set is closed")
        self._call("wfa_hip_pileup_add_quals", self._h, batch._h, _ptr(j), _ptr(t_start), _ptr(keep), _ptr(reverse), quals._h, _ptr(i),
                   _ptr(p_start), int(min_base_quality), int(quality_cap))

    def _rows(self, seq, start, length):
        """``(seq, start, length)`` as ints, a ``length`` of None running to the end of the sequence."""
        seq, start = int(seq), int(start)
        if length is None:
            if not 0 <= seq < self.n:
                raise ValueError(f"sequence {seq} is out of range for a set of {self.n}")
            length = int(self.length[seq]) - start
        return seq, start, int(length)

    def read(self, seq, start=0, length=None, strand=None):
        """wfa_hip_pileup_read: int32[length, 8], the rows [start, start + length) of one sequence (to its end when None).  ``strand``
        0 or 1: wfa_hip_pileup_read_strand, the forward or the reverse counts of a pileup that tracks strands."""
        seq, start, length = self._rows(seq, start, length)
        out = np.zeros((max(length, 0), PILEUP_COLS), np.int32)
        if strand is None:
            self._call("wfa_hip_pileup_read", self._h, seq, start, length, _ptr_or_null(out))
        else:
            self._call("wfa_hip_pileup_read_strand", self._h, seq, start, length, int(strand), _ptr_or_null(out))
        return out

    def read_quality(self, seq, start=0, length=None):
        """wfa_hip_pileup_read_quality: int32[length, 8], the rows of the quality table of a pileup that tracks qualities."""
        seq, start, length = self._rows(seq, start, length)
        out = np.zeros((max(length, 0), PILEUP_COLS), np.int32)
        self._call("wfa_hip_pileup_read_quality", self._h, seq, start, length, _ptr_or_null(out))
        return out

    def calls(self, texts, seq, start=0, length=None, min_depth=1):
        """wfa_hip_pileup_calls: uint8[length], the call bytes of the rows [start, start + length) of one sequence (to its end when
        None) against the letters of the SeqSet ``texts``."""
        seq, start, length = self._rows(seq, start, length)
        out = np.zeros(max(length, 0), np.uint8)
        self._call("wfa_hip_pileup_calls", self._h, texts._h, seq, start, length, int(min_depth), _ptr_or_null(out))
        return out

    def sites(self, texts, seq=-1, start=0, length=-1, min_depth=1, min_permille=500, cap=None):
        """wfa_hip_pileup_sites: ``(count, rows)``, rows int32 of shape (min(count, cap), 8) in ascending (j, pos); ``cap`` None: a
        counting call, then one with the exact capacity.  seq = -1: every sequence."""
        args = (self._h, texts._h, int(seq), int(start), int(length), int(min_depth), int(min_permille))
        count = ctypes.c_int64(0)
        if cap is None:
            self._call("wfa_hip_pileup_sites", *args, 0, ctypes.byref(count), None)
            cap = count.value
        rows = np.zeros((max(int(cap), 0), SITE_COLS), np.int32)
        if cap != 0:
            self._call("wfa_hip_pileup_sites", *args, int(cap), ctypes.byref(count), _ptr_or_null(rows))
        return count.value, rows[:min(count.value, rows.shape[0])]

    def genotypes(self, texts, seq=-1, start=0, length=-1, min_depth=1, min_permille=500, err_q=20, min_alt_strand=0, cap=None,
                  qualities=False):
        """wfa_hip_pileup_genotypes: ``(count, rows)``, rows int32 of shape (min(count, cap), 16) in ascending (j, pos); ``cap`` None: a
        counting call, then one with the exact capacity.  seq = -1: every sequence.  ``qualities``: wfa_hip_pileup_genotypes_quals,
        the costs from the quality table of a pileup that tracks qualities."""
        symbol = "wfa_hip_pileup_genotypes_quals" if qualities else "wfa_hip_pileup_genotypes"
        args = (self._h, texts._h, int(seq), int(start), int(length), int(min_depth), int(min_permille), int(err_q), int(min_alt_strand))
        count = ctypes.c_int64(0)
        if cap is None:
            self._call(symbol, *args, 0, ctypes.byref(count), None)
            cap = count.value
        rows = np.zeros((max(int(cap), 0), GENOTYPE_COLS), np.int32)
        if cap != 0:
            self._call(symbol, *args, int(cap), ctypes.byref(count), _ptr_or_null(rows))
        return count.value, rows[:min(count.value, rows.shape[0])]

    def clear(self):
        self._call("wfa_hip_pileup_clear", self._h)

    def track_strands(self, on=True):
        """wfa_hip_pileup_track_strands: keep (or stop keeping) the forward table; only while the pileup is empty."""
        self._call("wfa_hip_pileup_track_strands", self._h, 1 if on else 0)
        self.strands = bool(on)

    def track_qualities(self, on=True):
        """wfa_hip_pileup_track_qualities: keep (or stop keeping) the quality table; only while the pileup is empty."""
        self._call("wfa_hip_pileup_track_qualities", self._h, 1 if on else 0)
        self.qualities = bool(on)

    def track_insertions(self, on=True):
        """wfa_hip_pileup_track_insertions: keep (or stop keeping) what the reads insert; only while the pileup is empty."""
        self._call("wfa_hip_pileup_track_insertions", self._h, 1 if on else 0)
        self.tracking = bool(on)

    def insertion_stats(self):
        """wfa_hip_pileup_insertion_stats: ``(records, inserted bases)`` of the log."""
        records, bases = ctypes.c_int64(0), ctypes.c_int64(0)
        self._call("wfa_hip_pileup_insertion_stats", self._h, ctypes.byref(records), ctypes.byref(bases))
        return records.value, bases.value

    def insertions(self, texts, seq=-1, start=0, length=-1, min_depth=1, min_permille=500, cap=None, bases_cap=None):
        """wfa_hip_pileup_insertions: ``(count, rows, bases_count, bases)``; rows int32 of shape (min(count, cap), 8) in ascending
        (j, pos), bases the ASCII letters of the rows' alleles back to back (uint8, as many as were written).  A capacity of None: a
        counting call, then one with the exact capacities.  seq = -1: every sequence; min_permille = 0: the majority rule."""
        args = (self._h, texts._h, int(seq), int(start), int(length), int(min_depth), int(min_permille))
        count, nbases = ctypes.c_int64(0), ctypes.c_int64(0)
        if cap is None or bases_cap is None:
            self._call("wfa_hip_pileup_insertions", *args, 0, ctypes.byref(count), None, 0, ctypes.byref(nbases), None)
            cap = count.value if cap is None else cap
            bases_cap = nbases.value if bases_cap is None else bases_cap
        rows = np.zeros((max(int(cap), 0), INSERTION_COLS), np.int32)
        bases = np.zeros(max(int(bases_cap), 0), np.uint8)
        if cap != 0:
            self._call("wfa_hip_pileup_insertions", *args, int(cap), ctypes.byref(count), _ptr_or_null(rows), int(bases_cap),
                       ctypes.byref(nbases), _ptr_or_null(bases))
        rows = rows[:min(count.value, rows.shape[0])]
        return count.value, rows, nbases.value, bases[:_letters_written(rows, bases.shape[0])]


    def track_deletions(self, on=True):
        """wfa_hip_pileup_track_deletions: keep (or stop keeping) what the reads delete as runs; only while the pileup is empty."""
        self._call("wfa_hip_pileup_track_deletions", self._h, 1 if on else 0)
        self.deletions_tracked = bool(on)

    def deletion_stats(self):
        """wfa_hip_pileup_deletion_stats: ``(records, deleted bases)`` of the log."""
        records, bases = ctypes.c_int64(0), ctypes.c_int64(0)
        self._call("wfa_hip_pileup_deletion_stats", self._h, ctypes.byref(records), ctypes.byref(bases))
        return records.value, bases.value

    def deletion_starts(self, seq, start=0, length=None):
        """wfa_hip_pileup_read_deletion_starts: int32[length], the deletion records that start at each of the rows
        [start, start + length) of one sequence (to its end when None)."""
        seq, start, length = self._rows(seq, start, length)
        out = np.zeros(max(length, 0), np.int32)
        self._call("wfa_hip_pileup_read_deletion_starts", self._h, seq, start, length, _ptr_or_null(out))
        return out

    def deletions(self, texts, seq=-1, start=0, length=-1, min_depth=1, min_permille=500, cap=None):
        """wfa_hip_pileup_deletions: ``(count, rows)``, rows int32 of shape (min(count, cap), 8) in ascending (j, pos); ``cap`` None: a
        counting call, then one with the exact capacity.  seq = -1: every sequence; min_permille = 0: the majority rule."""
        args = (self._h, texts._h, int(seq), int(start), int(length), int(min_depth), int(min_permille))
        count = ctypes.c_int64(0)
        if cap is None:
            self._call("wfa_hip_pileup_deletions", *args, 0, ctypes.byref(count), None)
            cap = count.value
        rows = np.zeros((max(int(cap), 0), DELETION_COLS), np.int32)
        if cap != 0:
            self._call("wfa_hip_pileup_deletions", *args, int(cap), ctypes.byref(count), _ptr_or_null(rows))
        return count.value, rows[:min(count.value, rows.shape[0])]


class Placer(_Handle):
    """The hits of any number of batches, recorded and grouped by read in HBM (wfa_hip_placer_t); ``run`` reduces every read to one
    row.  Stays valid after the batches are closed."""

    _destroy = "wfa_hip_placer_destroy"

    def __init__(self, aligner, nreads):
        self.aligner = aligner
        self.nreads = int(nreads)
        self._created(lib().wfa_hip_placer_create(aligner._h, self.nreads), "wfa_hip_placer_create")

    def __len__(self):
        return int(lib().wfa_hip_placer_count(self._h))

    def add(self, batch, i, j, t_start=None, reverse=None):
        """wfa_hip_placer_add: the pairs of a ResidentBatch after its run, pair q a hit of read i[q] on texts[j[q]] from t_start[q]."""
        i = np.ascontiguousarray(i, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        t_start = None if t_start is None else np.ascontiguousarray(t_start, dtype=np.int32)
        reverse = None if reverse is None else np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
        for name, a in (("i", i), ("j", j), ("t_start", t_start), ("reverse", reverse)):
            if a is not None and a.shape != (batch.n,):
                raise ValueError(f"{name}: one value per pair of the batch ({batch.n})")
        self._call("wfa_hip_placer_add", self._h, batch._h, _ptr(i), _ptr(j), _ptr(t_start), _ptr(reverse))

    def add_hits(self, i, j, reverse, score, status, text_start, text_end, lead=None, trail=None):
        """wfa_hip_placer_add_hits: hits from host arrays, in list order.  ``lead`` / ``trail`` (int per hit, either None: 0):
        wfa_hip_placer_add_hits_clips, the hits' clips (not negative; saturated at CLIP_MAX)."""
        a, n = _hit_arrays(i, j, reverse, score, status, text_start, text_end)
        ptrs = [_ptr(a[k]) for k in ("i", "j", "reverse", "score", "status", "text_start", "text_end")]
        if lead is None and trail is None:
            self._call("wfa_hip_placer_add_hits", self._h, n, *ptrs)
        else:
            lead, trail = _clip_arrays(lead, trail, n)
            self._call("wfa_hip_placer_add_hits_clips", self._h, n, *ptrs, _ptr(lead), _ptr(trail))

    def clips(self):
        """wfa_hip_placer_read_clips: ``(lead, trail)``, int32 per hit added so far — the pattern bases in front of the first and behind
        the last M of each hit's alignment (0 under scope score)."""
        lead, trail = np.zeros(len(self), np.int32), np.zeros(len(self), np.int32)
        self._call("wfa_hip_placer_read_clips", self._h, _ptr_or_null(lead), _ptr_or_null(trail))
        return lead, trail

    def run(self, min_score=INT32_MIN, full_gap=1, flags=True):
        """wfa_hip_placer_run over every hit added so far: ``(rows, flags)``, rows int32 of shape (nreads, 8) in the columns
        PLACE_COLUMNS, flags uint8 per hit (None when ``flags`` is False)."""
        rows = np.zeros((self.nreads, PLACE_COLS), np.int32)
        fl = np.zeros(len(self), np.uint8) if flags else None
        self._call("wfa_hip_placer_run", self._h, int(min_score), int(full_gap), _ptr_or_null(rows), _ptr(fl))
        return rows, fl

    def run_pairs(self, mates, min_score=INT32_MIN, full_gap=1, min_insert=0, max_insert=1000, unpaired=0, rows=True, flags=True,
                  pair_flags=True):
        """wfa_hip_placer_run_pairs over every hit added so far: ``(rows, flags, pair_rows, pair_flags)`` — rows and flags as ``run``
        gives them, pair_rows int32 of shape (F, 12) in the columns PAIR_COLUMNS, pair_flags uint8 per hit; None for each of rows,
        flags and pair_flags that is False.  ``mates``: an (F, 2) integer array of read indices, or an int F: interleaved."""
        nfrag, m1, m2 = _mate_ptrs(mates)
        r = np.zeros((self.nreads, PLACE_COLS), np.int32) if rows else None
        fl = np.zeros(len(self), np.uint8) if flags else None
        pr = np.zeros((max(nfrag, 0), PAIR_COLS), np.int32)
        pf = np.zeros(len(self), np.uint8) if pair_flags else None
        p = _ptr_or_null
        self._call("wfa_hip_placer_run_pairs", self._h, int(min_score), int(full_gap), int(min_insert), int(max_insert), int(unpaired),
                   nfrag, m1, m2, p(r), p(fl), p(pr), p(pf))
        return r, fl, pr, pf

    def rescue(self, patterns, texts, mates, min_score=INT32_MIN, full_gap=1, min_insert=0, max_insert=1000, unpaired=0, pad=16, min_len=0,
               anchor_mapq=0, cap=None):
        """wfa_hip_placer_rescue over every hit added so far: ``(count, rows)`` of the windows in which the lost mates of the
        fragments without a proper pairing must lie — rows int32 of shape (min(count, cap), 8) in the columns RESCUE_COLUMNS, list
        order; ``cap`` None: room for every window (two per fragment).  ``patterns`` / ``texts``: the SeqSets of the reads and of the
        texts the hits lie on; ``mates`` as for ``run_pairs``."""
        nfrag, m1, m2 = _mate_ptrs(mates)
        if cap is None:
            cap = 2 * max(nfrag, 0)
        rows = np.zeros((max(int(cap), 0), RESCUE_COLS), np.int32)
        count = ctypes.c_int64(0)
        self._call("wfa_hip_placer_rescue", self._h, patterns._h, texts._h, int(min_score), int(full_gap), int(min_insert),
                   int(max_insert), int(unpaired), nfrag, m1, m2, int(pad), int(min_len), int(anchor_mapq), int(cap),
                   ctypes.byref(count), _ptr_or_null(rows))
        return count.value, rows[:min(count.value, rows.shape[0])]

    def duplicates(self, texts, mates, min_score=INT32_MIN, full_gap=1, min_insert=0, max_insert=1000, unpaired=0, unclipped=False,
                   qualities=None, min_quality=15):
        """wfa_hip_placer_duplicates over every hit added so far: ``(read_rows, pair_rows)``, int32 of shape (nreads, 4) and (F, 4)
        in the columns DUP_COLUMNS — the representative's number, the group's size, 1 for a duplicate, 1 for a bucket too full to
        resolve.  ``texts``: the SeqSet the hits lie on; ``mates`` as for ``run_pairs``, 0: the single-end form.  ``unclipped=True``
        (DUP_UNCLIPPED): keys and buckets on the hits' unclipped ends; ``qualities``, a QualSet over the placer's reads
        (DUP_BY_QUALITY): the representative is the unit with the greatest sum of base qualities of at least ``min_quality``.
        Either one: wfa_hip_placer_duplicates_ex."""
        nfrag, m1, m2 = _mate_ptrs(mates)
        read_rows = np.zeros((self.nreads, DUP_COLS), np.int32)
        pair_rows = np.zeros((max(nfrag, 0), DUP_COLS), np.int32)
        args = (self._h, texts._h, int(min_score), int(full_gap), int(min_insert), int(max_insert), int(unpaired), nfrag, m1, m2,
                _ptr_or_null(read_rows), _ptr_or_null(pair_rows))
        if not unclipped and qualities is None:
            self._call("wfa_hip_placer_duplicates", *args)
        else:
            if qualities is not None and not qualities._h:
                raise ValueError("the quality set is closed")
            flags = (DUP_UNCLIPPED if unclipped else 0) | (DUP_BY_QUALITY if qualities is not None else 0)
            self._call("wfa_hip_placer_duplicates_ex", *args, flags, None if qualities is None else qualities._h, int(min_quality))
        return read_rows, pair_rows

    def kernel_ms(self):
        ms = ctypes.c_float(0)
        self._call("wfa_hip_placer_kernel_ms", self._h, ctypes.byref(ms))
        return ms.value

    def clear(self):
        self._call("wfa_hip_placer_clear", self._h)


class SeedIndex(_Handle):
    """An exact-match k-mer index over a text SeqSet, resident in HBM (wfa_hip_seed_index_t): 4^k * 4 bytes of table plus 8 bytes per
    indexed position.  Stays valid after the set is closed."""

    _destroy = "wfa_hip_seed_index_destroy"

    def __init__(self, aligner, texts, k=13, stride=1, max_occ=64, w=None):
        if not texts._h:
            raise ValueError("sequence set is closed")
        self.aligner = aligner
        self.n = texts.n
        if w is None:
            self._created(lib().wfa_hip_seed_index_create(aligner._h, texts._h, k, stride, max_occ), "wfa_hip_seed_index_create")
        else:
            self._created(lib().wfa_hip_seed_index_create_minimizer(aligner._h, texts._h, k, w, max_occ),
                          "wfa_hip_seed_index_create_minimizer")

    def params(self):
        """wfa_hip_seed_index_params: dict(k=, stride=, w=); w = 0 for a stride index, stride = 1 for a minimizer index."""
        if not self._h:
            raise ValueError("seed index is closed")
        k, stride, w = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._call("wfa_hip_seed_index_params", self._h, ctypes.byref(k), ctypes.byref(stride), ctypes.byref(w))
        return dict(k=k.value, stride=stride.value, w=w.value)

    def query(self, patterns, n=4, min_hits=2, gap=16, pad=16, max_hits=2048):
        """wfa_hip_seed_index_query: dict of int32[M, n] ``j`` / ``reverse`` / ``text_start`` / ``text_len`` / ``hits`` and uint8[M]
        ``overflow`` for the M sequences of a SeqSet."""
        if not self._h:
            raise ValueError("seed index is closed")
        if not patterns._h:
            raise ValueError("sequence set is closed")
        cols = n if 1 <= n <= SEED_MAX_N else 1   # (out of range: the library refuses before it writes)
        out = {key: np.zeros((patterns.n, cols), np.int32) for key in SEED_KEYS}
        out["overflow"] = np.zeros(patterns.n, np.uint8)
        self._call("wfa_hip_seed_index_query", self._h, patterns._h, n, min_hits, gap, pad, max_hits,
                   *[_ptr(out[key]) for key in SEED_KEYS], _ptr(out["overflow"]))
        return out

    def chain(self, patterns, n=4, min_hits=3, min_score=40, lookback=32, max_dist=5000, band=500, pad=64, max_anchors=16384):
        """wfa_hip_seed_index_chain: dict of int32[M, n] per key of ``CHAIN_KEYS`` and uint8[M] ``overflow`` for the M sequences of a
        SeqSet."""
        if not self._h:
            raise ValueError("seed index is closed")
        if not patterns._h:
            raise ValueError("sequence set is closed")
        cols = n if 1 <= n <= SEED_MAX_N else 1   # (out of range: the library refuses before it writes)
        out = {key: np.zeros((patterns.n, cols), np.int32) for key in CHAIN_KEYS}
        out["overflow"] = np.zeros(patterns.n, np.uint8)
        self._call("wfa_hip_seed_index_chain", self._h, patterns._h, n, min_hits, min_score, lookback, max_dist, band, pad, max_anchors,
                   *[_ptr(out[key]) for key in CHAIN_KEYS], _ptr(out["overflow"]))
        return out

    def chain_stats(self):
        """wfa_hip_seed_index_chain_stats: dict(kernel_ms=, workspace_bytes=)."""
        if not self._h:
            raise ValueError("seed index is closed")
        ms, nbytes = ctypes.c_float(0), ctypes.c_int64(0)
        self._call("wfa_hip_seed_index_chain_stats", self._h, ctypes.byref(ms), ctypes.byref(nbytes))
        return dict(kernel_ms=ms.value, workspace_bytes=nbytes.value)

    def stats(self):
        """wfa_hip_seed_index_stats: dict(positions=, masked_kmers=, table_bytes=, build_ms=, query_ms=)."""
        if not self._h:
            raise ValueError("seed index is closed")
        pos, masked, nbytes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        bms, qms = ctypes.c_float(0), ctypes.c_float(0)
        self._call("wfa_hip_seed_index_stats", self._h, ctypes.byref(pos), ctypes.byref(masked), ctypes.byref(nbytes), ctypes.byref(bms),
                   ctypes.byref(qms))
        return dict(positions=pos.value, masked_kmers=masked.value, table_bytes=nbytes.value, build_ms=bms.value, query_ms=qms.value)


class MultiAligner(_Handle):
    """One aligner per device of a node (wfa_hip_multi_t): a batch is sharded over them, results land in disjoint
    slices of one set of arrays.  A handle of no aligner: it is created like one and keeps its own last error."""

    _destroy = "wfa_hip_multi_destroy"

    def __init__(self, cfg, devices):
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        self._h = lib().wfa_hip_multi_create(ctypes.byref(cfg), arr, len(self.devices))
        if not self._h:
            _raise_config_refused(cfg, "wfa_hip_multi_create")

    def _raise(self, rc, what):
        _raise_code(rc, what, lib().wfa_hip_multi_last_error(self._h).decode())

    def set_config(self, cfg):
        self._call("wfa_hip_multi_set_config", self._h, ctypes.byref(cfg))

    def align_batch(self, batch, want_cigar):
        if "packed" in batch:   # (the multi-device entry takes ASCII; 2-bit bytes would be read as letters outside ACGT)
            raise NotImplementedError("wfa_hip_multi_align_batch takes ASCII reads: 2-bit batches go through Aligner.align_batch per device")
        seqs, p_off, p_len, t_off, t_len, n = _check_batch(batch)
        score = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        if want_cigar:
            cigar_off = np.zeros(n + 1, np.int64)
            np.cumsum(p_len.astype(np.int64) + t_len.astype(np.int64), out=cigar_off[1:])
            ops = np.zeros(max(int(cigar_off[-1]), 1), np.uint8)
            cbeg = np.zeros(n, np.int64)
            clen = np.zeros(n, np.int32)
        else:
            cigar_off = ops = cbeg = clen = None
        self._call("wfa_hip_multi_align_batch", self._h, n, _ptr(seqs), _ptr(p_off), _ptr(p_len), _ptr(t_off), _ptr(t_len),
                   _ptr(score), _ptr(status), _ptr(ops), _ptr(cigar_off), _ptr(cbeg), _ptr(clen))
        return score, status, ((ops, cbeg, clen) if want_cigar else None)


class ResidentBatch(_Handle):
    """A batch kept in HBM (wfa_hip_batch_t): upload + 2-bit pack once, run many times."""

    _destroy = "wfa_hip_batch_destroy"
    _device_failure = "failed:"   # (a batch's create tells a device failure by the HIP_TRY form only, as it always did)

    def __init__(self, aligner, batch):
        seqs, p_off, p_len, t_off, t_len, n = _check_batch(batch)
        self.aligner = aligner
        self.n = n
        self._p_len, self._t_len = p_len, t_len
        create = lib().wfa_hip_batch_create_packed2bits if "packed" in batch else lib().wfa_hip_batch_create
        self._created(create(aligner._h, n, _ptr(seqs), _ptr(p_off), _ptr(p_len), _ptr(t_off), _ptr(t_len)), "wfa_hip_batch_create")

    @classmethod
    def indexed(cls, aligner, patterns, texts, i, j):
        """wfa_hip_batch_create_indexed over two SeqSets (texts None: both indices into ``patterns``).  ``i`` / ``j``: integer arrays
        of equal length, every value inside its set (the library checks them again and raises ValueError)."""
        for a in (np.asarray(i), np.asarray(j)):
            if a.size and (a.dtype.kind not in "iu" or
                           (a.dtype != np.int32 and (int(a.min()) < -2**31 or int(a.max()) >= 2**31))):
                raise ValueError("index arrays must hold integers that fit 32 bits")
        i = np.ascontiguousarray(i, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        if i.ndim != 1 or i.shape != j.shape:
            raise ValueError("index arrays differ in length")
        tset = patterns if texts is None else texts
        if not patterns._h or not tset._h:
            raise ValueError("sequence set is closed")
        self = cls.__new__(cls)
        self.aligner = aligner
        self.n = n = i.shape[0]
        # (the pairs' lengths, which size the op buffers of results(True), are looked up when first asked for: the library has
        # checked the indices by then)
        self._lens = (patterns.length, tset.length, i, j)
        h = lib().wfa_hip_batch_create_indexed(aligner._h, patterns._h, texts._h if texts is not None else None, n, _ptr(i), _ptr(j))
        self._created(h, "wfa_hip_batch_create_indexed")
        return self

    @classmethod
    def windows(cls, aligner, patterns, texts, i, j, p_start=None, p_len=None, t_start=None, t_len=None, reverse=None):
        """wfa_hip_batch_create_windows over two SeqSets (texts None: both indices into ``patterns``).  ``i`` / ``j`` and the optional
        start / length arrays: integers that fit 32 bits, one per pair; ``reverse``: 0 / 1 per pair.  None = the C entry's NULL.  A
        list the library refuses raises NativeError carrying its message."""
        given = {"i": i, "j": j, "p_start": p_start, "p_len": p_len, "t_start": t_start, "t_len": t_len}
        arr = {}
        for name, a in given.items():
            if a is None:
                if name in ("i", "j"):
                    raise ValueError("index arrays are missing")
                arr[name] = None
                continue
            a = np.asarray(a)
            if a.size and (a.dtype.kind not in "iu" or
                           (a.dtype != np.int32 and (int(a.min()) < -2**31 or int(a.max()) >= 2**31))):
                raise ValueError(f"{name} must hold integers that fit 32 bits")
            arr[name] = np.ascontiguousarray(a, dtype=np.int32)
        if reverse is not None:
            arr["reverse"] = np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
        else:
            arr["reverse"] = None
        n = arr["i"].shape[0]
        for name, a in arr.items():
            if a is not None and (a.ndim != 1 or a.shape[0] != n):
                raise ValueError(f"window arrays differ in length ({name})")
        tset = patterns if texts is None else texts
        if not patterns._h or not tset._h:
            raise ValueError("sequence set is closed")
        self = cls.__new__(cls)
        self.aligner = aligner
        self.n = n
        self._wins = (patterns.length, tset.length, arr)   # (the windows' lengths size the op buffers of results(True): on first use)
        h = lib().wfa_hip_batch_create_windows(aligner._h, patterns._h, texts._h if texts is not None else None, n,
                                               *[_ptr(arr[k]) for k in ("i", "j", "p_start", "p_len", "t_start", "t_len", "reverse")])
        self._created(h, "wfa_hip_batch_create_windows", refused=NativeError)
        return self

    def __getattr__(self, name):
        if name in ("_p_len", "_t_len") and "_wins" in self.__dict__:   # a windowed batch: the listed windows' lengths, on first use
            pl, tl, a = self._wins
            ps = a["p_start"] if a["p_start"] is not None else 0
            ts = a["t_start"] if a["t_start"] is not None else 0
            self._p_len = a["p_len"] if a["p_len"] is not None else (pl[a["i"]] - ps).astype(np.int32)
            self._t_len = a["t_len"] if a["t_len"] is not None else (tl[a["j"]] - ts).astype(np.int32)
            return self.__dict__[name]
        if name in ("_p_len", "_t_len") and "_lens" in self.__dict__:   # an indexed batch: the listed pairs' lengths, on first use
            pl, tl, i, j = self._lens
            self._p_len, self._t_len = pl[i], tl[j]
            return self.__dict__[name]
        raise AttributeError(name)

    def run(self, stream=None):
        self._call("wfa_hip_batch_run", self._h, stream)

    def sync(self):
        self._call("wfa_hip_batch_sync", self._h)

    def results(self, want_cigar):
        n = self.n
        score = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        if want_cigar:
            cigar_off = np.zeros(n + 1, np.int64)
            np.cumsum(self._p_len.astype(np.int64) + self._t_len.astype(np.int64), out=cigar_off[1:])
            ops = np.zeros(max(int(cigar_off[-1]), 1), np.uint8)
            cbeg = np.zeros(n, np.int64)
            clen = np.zeros(n, np.int32)
        else:
            cigar_off = ops = cbeg = clen = None
        self._call("wfa_hip_batch_results", self._h, _ptr(score), _ptr(status), _ptr(ops), _ptr(cigar_off), _ptr(cbeg), _ptr(clen))
        return score, status, ((ops, cbeg, clen) if want_cigar else None)

    def last_kernel(self):
        ms = ctypes.c_float(0)
        pairs = ctypes.c_int64(0)
        self._call("wfa_hip_batch_last_kernel_ms", self._h, ctypes.byref(ms), ctypes.byref(pairs))
        return ms.value, pairs.value

    def rle(self):
        """cigartuples + locations of the whole batch, computed on the GPU.

        Returns run_off int64[n+1], run_code uint8[total], run_len int32[total], locations int32[n,4]."""
        n = self.n
        cnt = np.zeros(n, np.int32)
        locs = np.zeros((n, 4), np.int32)
        total = lib().wfa_hip_batch_rle_counts(self._h, _ptr(cnt), _ptr(locs))
        if total < 0:
            self._raise(int(total), "wfa_hip_batch_rle_counts")
        code = np.zeros(max(int(total), 1), np.uint8)
        rlen = np.zeros(max(int(total), 1), np.int32)
        self._call("wfa_hip_batch_rle_runs", self._h, _ptr(code), _ptr(rlen))
        off = np.zeros(n + 1, np.int64)
        np.cumsum(cnt, out=off[1:])
        return off, code[:total], rlen[:total], locs

    def summary(self):
        """wfa_hip_batch_summary: int32[n, 10] of the last scope=full run, reduced on the GPU — per pair the numbers of M, X, I and D
        ops, of I runs and of D runs, and the four ``locations``."""
        out = np.zeros((self.n, SUMMARY_COLS), np.int32)
        self._call("wfa_hip_batch_summary", self._h, _ptr(out) if self.n else None)
        return out

    def left_align(self):
        """wfa_hip_batch_left_align: the op strings of the status-0 pairs of the last scope=full run rewritten in place on the GPU, every
        gap run at the left end of its repeat; everything read from the batch afterwards sees them.  Returns (runs moved, merges)."""
        stats = np.zeros(2, np.int64)
        self._call("wfa_hip_batch_left_align", self._h, _ptr(stats))
        return int(stats[0]), int(stats[1])

    def sam(self, flags=0):
        """wfa_hip_batch_sam_counts and _sam_strings: the SAM fields of the last scope=full run, made on the GPU (after a
        ``left_align()``: of the rewritten strings).  Returns (rows int32[n, 8] in the columns SAM_COLUMNS, the CIGAR strings and the MD
        strings as two uint8 blobs): pair q's strings start at the prefix sums of columns 5 and 6.  ``flags``: SAM_EQX | SAM_CORE."""
        rows = np.zeros((self.n, SAM_COLS), np.int32)
        nc, nm = ctypes.c_int64(0), ctypes.c_int64(0)
        self._call("wfa_hip_batch_sam_counts", self._h, int(flags), _ptr(rows) if self.n else None, ctypes.byref(nc), ctypes.byref(nm))
        cigar, md = np.zeros(max(nc.value, 1), np.uint8), np.zeros(max(nm.value, 1), np.uint8)
        self._call("wfa_hip_batch_sam_strings", self._h, _ptr(cigar), _ptr(md))
        return rows, cigar[:nc.value], md[:nm.value]

    def sam_kernel_ms(self):
        """wfa_hip_batch_sam_kernel_ms: the HIP-event time of the two passes of the last ``sam()``."""
        ms = ctypes.c_float(0)
        self._call("wfa_hip_batch_sam_kernel_ms", self._h, ctypes.byref(ms))
        return ms.value

    def algorithmic_bytes(self):
        return int(lib().wfa_hip_batch_algorithmic_bytes(self._h))

    def fallback_pairs(self):
        return int(lib().wfa_hip_batch_fallback_pairs(self._h))
