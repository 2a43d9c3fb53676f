"""ctypes binding of the C-ABI in include/quicked.h + include/quicked_batch.h.

Loads ``quicked_amd/libquicked_hip.so`` (built in-tree by ``build.py``) and
fails loudly when it is missing: there is no Python or CPU fallback path.
"""
import ctypes as C
import os

import numpy as np

from . import build

QUICKED, WINDOWED, BANDED, HIRSCHBERG = 0, 1, 2, 3
QUICKED_OK, QUICKED_ERROR, QUICKED_FAIL_NON_CONVERGENCE = 0, -1, -2
QUICKED_UNKNOWN_ALGO, QUICKED_EMPTY_SEQUENCE, QUICKED_UNIMPLEMENTED, QUICKED_WIP = -3, -4, -10, 1


class ProfilerCounter(C.Structure):
    _fields_ = [("total", C.c_uint64), ("samples", C.c_uint64), ("min", C.c_uint64), ("max", C.c_uint64),
                ("m_oldM", C.c_double), ("m_newM", C.c_double), ("m_oldS", C.c_double), ("m_newS", C.c_double)]


class Timespec(C.Structure):
    _fields_ = [("tv_sec", C.c_long), ("tv_nsec", C.c_long)]


class ProfilerTimer(C.Structure):
    _fields_ = [("begin_timer", Timespec), ("time_ns", ProfilerCounter), ("accumulated", C.c_uint64)]


class MMAllocator(C.Structure):
    _fields_ = [("request_ticker", C.c_uint64), ("segment_size", C.c_uint64), ("segments", C.c_void_p),
                ("segments_free", C.c_void_p), ("current_segment_idx", C.c_uint64),
                ("malloc_requests", C.c_void_p), ("malloc_requests_freed", C.c_uint64)]


class Params(C.Structure):
    """quicked_params_t (include/quicked.h; reference quicked/quicked.h:43-54)"""
    _fields_ = [("algo", C.c_int), ("bandwidth", C.c_uint), ("window_size", C.c_uint), ("overlap_size", C.c_uint),
                ("hew_threshold", C.c_uint * 2), ("hew_percentage", C.c_uint * 2),
                ("only_score", C.c_bool), ("force_scalar", C.c_bool), ("external_timer", C.c_bool),
                ("external_allocator", C.POINTER(MMAllocator))]


class Aligner(C.Structure):
    """quicked_aligner_t (include/quicked.h; reference quicked/quicked.h:56-67)"""
    _fields_ = [("params", C.POINTER(Params)), ("mm_allocator", C.POINTER(MMAllocator)), ("cigar", C.c_char_p),
                ("score", C.c_int), ("timer", C.POINTER(ProfilerTimer)),
                ("timer_windowed_s", C.POINTER(ProfilerTimer)), ("timer_windowed_l", C.POINTER(ProfilerTimer)),
                ("timer_banded", C.POINTER(ProfilerTimer)), ("timer_align", C.POINTER(ProfilerTimer))]


EXPORTS = ["quicked_check_error", "quicked_status_msg", "quicked_default_params", "quicked_new", "quicked_free",
           "quicked_align", "quicked_set_device", "quicked_device_count", "quicked_align_batch", "quicked_batch_create",
           "quicked_batch_destroy", "quicked_batch_run", "quicked_batch_sync", "quicked_batch_scores",
           "quicked_batch_cigar_bytes", "quicked_batch_cigars", "quicked_batch_counters",
           "quicked_batch_kernel_time", "quicked_batch_kernel_times", "quicked_host_alloc", "quicked_host_free",
           "quicked_batch_configure", "quicked_batch_check_results", "quicked_batch_validate",
           "quicked_wire_words", "quicked_wire_pack", "quicked_batch_create_packed",
           "quicked_batch_reload", "quicked_batch_reload_packed", "quicked_batch_fetch", "quicked_pool_stats", "quicked_batch_cigar_view",
           "quicked_batch_deferred_pairs", "quicked_wire_pack_pool", "quicked_wire_offsets", "quicked_wire_pack_isa", "quicked_pool_trim", "quicked_early_finish_stats",
           "quicked_batch_run_bounded", "quicked_batch_run_search", "quicked_batch_locations",
           "quicked_batch_run_search_all", "quicked_batch_hit_counts", "quicked_batch_hit_total", "quicked_batch_hits",
           "quicked_batch_run_panel", "quicked_batch_panel_results", "quicked_batch_panel_matrix",
           "quicked_batch_run_panel_all", "quicked_batch_run_panel_scan", "quicked_batch_panel_hit_counts", "quicked_batch_panel_hit_total", "quicked_batch_panel_hits",
           "quicked_batch_panel_hit_cigar_bytes", "quicked_batch_panel_hit_cigars",
           "quicked_batch_configure_panel_tails", "quicked_batch_panel_tails",
           "quicked_batch_configure_panel_heads", "quicked_batch_panel_heads",
           "quicked_batch_configure_panel_queue", "quicked_batch_panel_queue_wanted",
           "quicked_batch_run_panel_scan_no_indels",
           "quicked_batch_configure_tags", "quicked_batch_pair_stats", "quicked_batch_md_bytes", "quicked_batch_md"]

TAG_STATS, TAG_MD, TAG_NO_CIGAR = 1, 2, 4
HIT_DTYPE = np.dtype([("text_start", np.int32), ("text_end", np.int32), ("score", np.int32)])      # quicked_hit_t
SEARCH_PREFIX, SEARCH_INFIX = 1, 2
SEARCH_IUPAC, SEARCH_IUPAC_PATTERN = 16, 32      # OR-ed into a search mode: IUPAC base sets on both sides / on the pattern only
PANEL_MATRIX = 64                                # OR-ed into a panel run's mode: keep every {score, text_end}
PANEL_CIGARS = 512                               # OR-ed into run_panel_all's / run_panel_scan's mode: every stored occurrence's alignment
PANEL_TAILS = 2048                               # OR-ed into run_panel_all's mode: every text's 3' tail besides (panel_tails())
PANEL_HEADS = 8192                               # OR-ed into run_panel_all's mode: every text's 5' head besides (panel_heads())
PANEL_NO_INDELS = 32768                          # OR-ed into run_panel's / run_panel_all's mode: mismatches only, text_start = text_end - m
PANEL_MAX_PATTERNS, PANEL_MAX_LEN = 4096, 256
PANEL_HIT_DTYPE = np.dtype([("pattern", np.int32), ("score", np.int32), ("text_start", np.int32), ("text_end", np.int32),
                            ("second_pattern", np.int32), ("second_score", np.int32)])      # quicked_panel_hit_t
PANEL_OCC_DTYPE = np.dtype([("pattern", np.int32), ("text_start", np.int32), ("text_end", np.int32), ("score", np.int32)])      # quicked_panel_occ_t
PANEL_TAIL_DTYPE = np.dtype([("pattern", np.int32), ("overlap", np.int32), ("text_start", np.int32), ("score", np.int32)])      # quicked_panel_tail_t
PANEL_HEAD_DTYPE = np.dtype([("pattern", np.int32), ("overlap", np.int32), ("text_end", np.int32), ("score", np.int32)])      # quicked_panel_head_t

_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("QUICKED_HIP_LIB") or build.HIP_LIB       # A/B runs of two builds: QUICKED_HIP_LIB=<other .so>
    if not os.path.exists(path):
        try:
            build.build_hip()            # hipcc --offload-arch=gfx950, in-tree
        except Exception as e:           # noqa: BLE001
            raise RuntimeError(f"{path} is missing and could not be built ({e}): run "
                               "`python -c 'import __graft_entry__ as g; g.build()'`; there is no fallback path") from e
    # The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that
    # share one serialise; a thread's runs rotate over up to 12 stream sets.  The runtime reads the variable when it
    # initialises, so the embedding application sets it before its first HIP call; this binding is one.
    # 20: with 24 queues in existence the hardware oversubscribes and small-batch streams lose a third of their rate.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")
    L = C.CDLL(path)
    L.quicked_check_error.restype = C.c_bool
    L.quicked_check_error.argtypes = [C.c_int]
    L.quicked_status_msg.restype = C.c_char_p
    L.quicked_status_msg.argtypes = [C.c_int]
    L.quicked_default_params.restype = Params
    L.quicked_default_params.argtypes = []
    L.quicked_new.argtypes = [C.POINTER(Aligner), C.POINTER(Params)]
    L.quicked_free.argtypes = [C.POINTER(Aligner)]
    L.quicked_align.argtypes = [C.POINTER(Aligner), C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    L.quicked_set_device.argtypes = [C.c_int]
    L.quicked_align_batch.argtypes = [C.POINTER(Aligner), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                      C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
    L.quicked_batch_create.restype = C.c_void_p
    L.quicked_batch_create.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_destroy.argtypes = [C.c_void_p]
    L.quicked_batch_destroy.restype = None
    L.quicked_batch_run.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int]
    L.quicked_batch_run_bounded.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int]
    L.quicked_batch_run_bounded.restype = C.c_int
    L.quicked_batch_run_search.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int, C.c_int]
    L.quicked_batch_run_search.restype = C.c_int
    L.quicked_batch_locations.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_locations.restype = C.c_int
    L.quicked_batch_run_search_all.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int]
    L.quicked_batch_run_search_all.restype = C.c_int
    L.quicked_batch_hit_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_hit_counts.restype = C.c_int
    L.quicked_batch_hit_total.argtypes = [C.c_void_p]
    L.quicked_batch_hit_total.restype = C.c_int64
    L.quicked_batch_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_hits.restype = C.c_int
    L.quicked_batch_run_panel.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int]
    L.quicked_batch_run_panel.restype = C.c_int
    L.quicked_batch_panel_results.argtypes = [C.c_void_p, C.c_void_p]
    L.quicked_batch_panel_results.restype = C.c_int
    L.quicked_batch_panel_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_panel_matrix.restype = C.c_int
    L.quicked_batch_run_panel_all.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int]
    L.quicked_batch_run_panel_all.restype = C.c_int
    L.quicked_batch_run_panel_scan.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int]
    L.quicked_batch_run_panel_scan.restype = C.c_int
    if hasattr(L, "quicked_batch_run_panel_scan_no_indels"):      # (an older build loaded for an A/B run lacks the newer symbols)
        L.quicked_batch_run_panel_scan_no_indels.argtypes = L.quicked_batch_run_panel_scan.argtypes
        L.quicked_batch_run_panel_scan_no_indels.restype = C.c_int
    L.quicked_batch_panel_hit_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_panel_hit_counts.restype = C.c_int
    L.quicked_batch_panel_hit_total.argtypes = [C.c_void_p]
    L.quicked_batch_panel_hit_total.restype = C.c_int64
    L.quicked_batch_panel_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_panel_hits.restype = C.c_int
    if hasattr(L, "quicked_batch_panel_hit_cigars"):      # (an older build loaded for an A/B run lacks the newer symbols)
        L.quicked_batch_panel_hit_cigar_bytes.argtypes = [C.c_void_p]
        L.quicked_batch_panel_hit_cigar_bytes.restype = C.c_int64
        L.quicked_batch_panel_hit_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.quicked_batch_panel_hit_cigars.restype = C.c_int
    if hasattr(L, "quicked_batch_panel_tails"):           # (as above)
        L.quicked_batch_configure_panel_tails.argtypes = [C.c_void_p, C.c_int32]
        L.quicked_batch_configure_panel_tails.restype = C.c_int
        L.quicked_batch_panel_tails.argtypes = [C.c_void_p, C.c_void_p]
        L.quicked_batch_panel_tails.restype = C.c_int
    if hasattr(L, "quicked_batch_panel_heads"):           # (as above)
        L.quicked_batch_configure_panel_heads.argtypes = [C.c_void_p, C.c_int32]
        L.quicked_batch_configure_panel_heads.restype = C.c_int
        L.quicked_batch_panel_heads.argtypes = [C.c_void_p, C.c_void_p]
        L.quicked_batch_panel_heads.restype = C.c_int
    if hasattr(L, "quicked_batch_configure_panel_queue"):      # (as above)
        L.quicked_batch_configure_panel_queue.argtypes = [C.c_void_p, C.c_int64]
        L.quicked_batch_configure_panel_queue.restype = C.c_int
        L.quicked_batch_panel_queue_wanted.argtypes = [C.c_void_p]
        L.quicked_batch_panel_queue_wanted.restype = C.c_int64
    L.quicked_batch_sync.argtypes = [C.c_void_p]
    L.quicked_batch_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_cigar_bytes.restype = C.c_int64
    L.quicked_batch_cigar_bytes.argtypes = [C.c_void_p]
    L.quicked_batch_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_counters.argtypes = [C.c_void_p, C.c_void_p]
    L.quicked_batch_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    if hasattr(L, "quicked_batch_kernel_times"):      # (an older build loaded through QUICKED_HIP_LIB for an A/B run lacks the newer symbols)
        L.quicked_batch_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_configure.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.quicked_batch_check_results.argtypes = [C.c_void_p, C.c_void_p]
    L.quicked_batch_validate.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.quicked_batch_configure_tags.argtypes = [C.c_void_p, C.c_int]
    L.quicked_batch_pair_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.quicked_batch_md_bytes.restype = C.c_int64
    L.quicked_batch_md_bytes.argtypes = [C.c_void_p]
    L.quicked_batch_md.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_debug_tag_launches.argtypes = [C.c_void_p]
    if hasattr(L, "quicked_debug_pack"):
        L.quicked_debug_pack.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.quicked_wire_words.restype = C.c_int64
    L.quicked_wire_words.argtypes = [C.c_int32, C.c_int]
    L.quicked_wire_pack.argtypes = [C.c_char_p, C.c_int32, C.c_int, C.c_void_p]
    L.quicked_batch_create_packed.restype = C.c_void_p
    L.quicked_batch_create_packed.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_reload.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_reload_packed.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.quicked_batch_fetch.argtypes = [C.c_void_p]
    L.quicked_pool_stats.argtypes = [C.c_void_p]
    if hasattr(L, "quicked_early_finish_stats"):
        L.quicked_early_finish_stats.argtypes = [C.c_void_p]
    L.quicked_batch_cigar_view.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.quicked_batch_deferred_pairs.restype = C.c_int64
    L.quicked_batch_deferred_pairs.argtypes = [C.c_void_p]
    L.quicked_wire_pack_pool.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int64)]
    L.quicked_wire_offsets.restype = C.c_int64
    L.quicked_wire_offsets.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    L.quicked_wire_pack_isa.argtypes = [C.c_int]
    L.quicked_host_alloc.restype = C.c_void_p
    L.quicked_host_alloc.argtypes = [C.c_size_t]
    L.quicked_host_free.argtypes = [C.c_void_p]
    L.quicked_host_free.restype = None
    _LIB = L
    return L


def reload_env():
    """The library parses its QE_* switches once (qe_pool.h: SwitchTable); code that changes one in os.environ while the
    library is loaded -- the in-process parity tests that force a kernel form, bench.py's classic-flow leg -- calls this to
    have it parsed again.  No-op while the library is not loaded (its first use parses the environment as it is then)."""
    if _LIB is not None and hasattr(_LIB, "quicked_debug_reload_env"):
        _LIB.quicked_debug_reload_env()


def tag_launches():
    """count passes of the alignment-tag kernels launched by this process so far -> (lane form, wave form); a test hook"""
    v = np.zeros(2, dtype=np.int64)
    lib().quicked_debug_tag_launches(v.ctypes.data)
    return int(v[0]), int(v[1])


def debug_pack(patterns, texts, reverse=False):
    """k_pack's planes of two sets of byte strings of equal count, through the one launch that packs both; a test hook ->
    (pattern words, pattern word offsets, text words, text word offsets, flags per pair); words: uint64, 3 per 64 bases
    {code bit 0, code bit 1, not ACGT} and two rows of zeros behind every sequence"""
    assert len(patterns) == len(texts)
    n = len(patterns)

    def pool_of(seqs):
        length = np.array([len(s) for s in seqs], dtype=np.int32)
        off = np.zeros(n, dtype=np.int64)
        if n:
            off[1:] = np.cumsum(length[:-1], dtype=np.int64)
        pool = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
        return pool, off, length, int(sum(3 * ((int(v) + 63) // 64 + 2) for v in length))

    pp, po, pl, pw = pool_of(patterns)
    tp, to, tl, tw = pool_of(texts)
    p_words, t_words = np.zeros(pw + 1, dtype=np.uint64), np.zeros(tw + 1, dtype=np.uint64)
    p_off, t_off = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    flags = np.zeros(n + 1, dtype=np.uint32)
    st = lib().quicked_debug_pack(n, pp.ctypes.data, po.ctypes.data, pl.ctypes.data, tp.ctypes.data, to.ctypes.data, tl.ctypes.data,
                                  1 if reverse else 0, p_words.ctypes.data, pw, p_off.ctypes.data, t_words.ctypes.data, tw,
                                  t_off.ctypes.data, flags.ctypes.data)
    if st < 0:
        raise QuickedException(st)
    return p_words[:pw], p_off[:n], t_words[:tw], t_off[:n], flags[:n]


def pool_trim():
    """quicked_pool_trim: the calling thread's device pools go back to the device"""
    return lib().quicked_pool_trim()


def pool_stats():
    """quicked_pool_stats of the calling thread: dict(pool_bytes, reclaim_events, sets, sub_batches, pool_budget) plus the
    process-wide book: bytes all pools of the thread's device hold, contexts in existence, contexts on lease"""
    v = np.zeros(8, dtype=np.int64)
    lib().quicked_pool_stats(v.ctypes.data)
    return dict(pool_bytes=int(v[0]), reclaim_events=int(v[1]), sets=int(v[2]), sub_batches=int(v[3]), pool_budget=int(v[4]),
                device_pool_bytes=int(v[5]), contexts=int(v[6]), contexts_leased=int(v[7]))


def early_finish_stats():
    """quicked_early_finish_stats: dict(flows, batches, merged_flows, merged_batches)"""
    v = np.zeros(4, dtype=np.int64)
    lib().quicked_early_finish_stats(v.ctypes.data)
    return dict(flows=int(v[0]), batches=int(v[1]), merged_flows=int(v[2]), merged_batches=int(v[3]))


def make_params(**kw):
    p = lib().quicked_default_params()
    for k, v in kw.items():
        if k in ("hew_threshold", "hew_percentage"):
            getattr(p, k)[0], getattr(p, k)[1] = v
        else:
            setattr(p, k, v)
    return p


class QuickedException(Exception):
    def __init__(self, status):
        self.status = status
        super().__init__(lib().quicked_status_msg(status).decode())


class QuickedAligner:
    """Mirror of the reference's C++/Python binding (bindings/cpp/quicked.hpp:40-66,
    bindings/python/quicked.cpp:33-45): same method names, same behaviour."""

    def __init__(self):
        self._lib = lib()
        self._params = self._lib.quicked_default_params()
        self._aligner = Aligner()
        st = self._lib.quicked_new(C.byref(self._aligner), C.byref(self._params))
        if self._lib.quicked_check_error(st):
            raise QuickedException(st)

    def __del__(self):
        try:
            self._lib.quicked_free(C.byref(self._aligner))
        except Exception:
            pass

    def align(self, pattern, text):
        pattern = pattern.encode() if isinstance(pattern, str) else pattern
        text = text.encode() if isinstance(text, str) else text
        st = self._lib.quicked_align(C.byref(self._aligner), pattern, len(pattern), text, len(text))
        if self._lib.quicked_check_error(st):
            raise QuickedException(st)
        return st

    def setAlgorithm(self, algo): self._params.algo = int(algo)
    def setOnlyScore(self, v): self._params.only_score = bool(v)
    def setBandwidth(self, v): self._params.bandwidth = int(v)
    def setWindowSize(self, v): self._params.window_size = int(v)
    def setOverlapSize(self, v): self._params.overlap_size = int(v)
    def setForceScalar(self, v): self._params.force_scalar = bool(v)

    def setHEWThreshold(self, v):
        self._params.hew_threshold[0] = self._params.hew_threshold[1] = int(v)

    def setHEWPercentage(self, v):
        self._params.hew_percentage[0] = self._params.hew_percentage[1] = int(v)

    def getScore(self): return self._aligner.score
    def getCigar(self): return self._aligner.cigar.decode() if self._aligner.cigar else "NULL"

    # additive: the batch entry point
    def alignBatch(self, pairs):
        n = len(pairs)
        pats = (C.c_char_p * n)(*[p for p, _ in pairs])
        txts = (C.c_char_p * n)(*[t for _, t in pairs])
        pl = (C.c_int * n)(*[len(p) for p, _ in pairs])
        tl = (C.c_int * n)(*[len(t) for _, t in pairs])
        scores = (C.c_int * n)(*([-1] * n))
        status = (C.c_int * n)()
        cigs = (C.c_char_p * n)()
        want = not self._params.only_score
        st = self._lib.quicked_align_batch(C.byref(self._aligner), n, pats, pl, txts, tl, scores,
                                           cigs if want else None, status)
        out = [(status[i], scores[i], (cigs[i].decode() if (want and cigs[i]) else None)) for i in range(n)]
        return st, out


WIRE_2BIT, WIRE_PLANES3 = 2, 3


def wire_offsets(length, wire):
    """dense word layout of sequences of these lengths: -> (int64 word offsets, total words)"""
    length = np.ascontiguousarray(length, dtype=np.int32)
    woff = np.zeros(len(length), dtype=np.int64)
    total = lib().quicked_wire_offsets(len(length), length.ctypes.data, wire, woff.ctypes.data)
    if total < 0:
        raise QuickedException(QUICKED_ERROR)
    return woff, int(total)


def wire_pack_pool(pool, off, length, wire, threads=0, out=None):
    """host-side serializer over a byte pool, one C call (quicked_wire_pack_pool: SIMD, multi-threaded): -> (uint64 words
    back to back, word offsets); `out` = a preallocated uint64 array (e.g. pinned) to pack into.  QuickedException if a
    sequence holds a symbol the wire format cannot represent."""
    L = lib()
    length = np.ascontiguousarray(length, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    woff, total = wire_offsets(length, wire)
    words = out if out is not None else np.zeros(total + 1, dtype=np.uint64)
    assert words.dtype == np.uint64 and len(words) >= total
    bad = C.c_int64(-1)
    st = L.quicked_wire_pack_pool(len(length), pool.ctypes.data, off.ctypes.data, length.ctypes.data, wire,
                                  words.ctypes.data, woff.ctypes.data, int(threads), C.byref(bad))
    if st < 0:
        raise QuickedException(st)
    return words, woff


class ResidentBatch:
    """quicked_batch_* : upload once, run many times (what bench.py times).  wire = WIRE_2BIT / WIRE_PLANES3 sends the
    packed form (quicked_batch_create_packed) instead of the ASCII pools."""

    def __init__(self, batch, wire=None):
        self._h = None
        self._lib = lib()
        self.n = len(batch)
        self._keep = batch
        if wire is None:
            self._h = self._lib.quicked_batch_create(
                self.n, batch.pattern_pool.ctypes.data, batch.pattern_off.ctypes.data, batch.pattern_len.ctypes.data,
                batch.text_pool.ctypes.data, batch.text_off.ctypes.data, batch.text_len.ctypes.data)
        else:
            pw, po = wire_pack_pool(batch.pattern_pool, batch.pattern_off, batch.pattern_len, wire)
            tw, to = wire_pack_pool(batch.text_pool, batch.text_off, batch.text_len, wire)
            self._wire = (pw, po, tw, to)
            self._h = self._lib.quicked_batch_create_packed(
                self.n, wire, pw.ctypes.data, po.ctypes.data, batch.pattern_len.ctypes.data,
                tw.ctypes.data, to.ctypes.data, batch.text_len.ctypes.data)
        if not self._h:
            raise RuntimeError("quicked_batch_create failed (no GPU / out of memory?)")

    @classmethod
    def from_wire(cls, batch, wire, pw, po, tw, to):
        """a batch from wire words that are already serialized (what a client holding packed data calls)"""
        self = cls.__new__(cls)
        self._lib = lib()
        self.n = len(batch)
        self._keep = (batch, pw, po, tw, to)
        self._h = self._lib.quicked_batch_create_packed(
            self.n, wire, pw.ctypes.data, po.ctypes.data, batch.pattern_len.ctypes.data,
            tw.ctypes.data, to.ctypes.data, batch.text_len.ctypes.data)
        if not self._h:
            raise RuntimeError("quicked_batch_create_packed failed")
        return self

    def run(self, params, sync=True):
        return self._lib.quicked_batch_run(self._h, C.byref(params), 1 if sync else 0)

    def run_bounded(self, max_dist, only_score=True, sync=True):
        """quicked_batch_run_bounded: per pair "the distance if it is <= its bound, else -1".  max_dist: one int for every
        pair, or an array of n bounds.  only_score=False (sync only): a CIGAR for every pair within its bound."""
        if np.ndim(max_dist) == 0:
            return self._lib.quicked_batch_run_bounded(self._h, None, int(max_dist), 1 if only_score else 0, 1 if sync else 0)
        md = np.ascontiguousarray(max_dist, dtype=np.int32)
        if md.shape != (self.n,):
            raise ValueError("max_dist: one bound per pair")
        return self._lib.quicked_batch_run_bounded(self._h, md.ctypes.data, 0, 1 if only_score else 0, 1 if sync else 0)

    def run_search(self, mode, max_dist=None, only_score=True, sync=True):
        """quicked_batch_run_search: where the pattern fits the text best (SEARCH_PREFIX: from the text's start, SEARCH_INFIX:
        anywhere) and at what cost.  max_dist: None = no bound, one int for every pair, or an array of n bounds.
        only_score=False (sync only): a CIGAR of the pattern against text[start:end] for every pair within its bound.
        mode | SEARCH_IUPAC reads both sequences as IUPAC base sets (equal when the sets intersect), mode | SEARCH_IUPAC_PATTERN
        the pattern only; such runs are score-and-location runs (only_score=False: QUICKED_UNIMPLEMENTED)."""
        if max_dist is None:
            max_dist = 2**31 - 1
        if np.ndim(max_dist) == 0:
            return self._lib.quicked_batch_run_search(self._h, int(mode), None, int(max_dist), 1 if only_score else 0, 1 if sync else 0)
        md = np.ascontiguousarray(max_dist, dtype=np.int32)
        if md.shape != (self.n,):
            raise ValueError("max_dist: one bound per pair")
        return self._lib.quicked_batch_run_search(self._h, int(mode), md.ctypes.data, 0, 1 if only_score else 0, 1 if sync else 0)

    def run_search_all(self, mode, max_dist=None, max_hits=16, sync=True):
        """quicked_batch_run_search_all: every occurrence of the pattern within the bound (the first columns of the valleys of
        row m), at most max_hits (1 .. 4096) stored per pair.  max_dist as in run_search.  Sync runs only.
        mode | SEARCH_IUPAC or mode | SEARCH_IUPAC_PATTERN: under the IUPAC base-set equality, as in run_search."""
        if max_dist is None:
            max_dist = 2**31 - 1
        if np.ndim(max_dist) == 0:
            return self._lib.quicked_batch_run_search_all(self._h, int(mode), None, int(max_dist), int(max_hits), 1 if sync else 0)
        md = np.ascontiguousarray(max_dist, dtype=np.int32)
        if md.shape != (self.n,):
            raise ValueError("max_dist: one bound per pair")
        return self._lib.quicked_batch_run_search_all(self._h, int(mode), md.ctypes.data, 0, int(max_hits), 1 if sync else 0)

    def hits(self):
        """-> (found, hit_off, hits) of the last all-occurrences run: found[i] occurrences of pair i (exact whatever the cap),
        the stored ones hits[hit_off[i]:hit_off[i + 1]], a structured array of HIT_DTYPE ordered by text_end.
        QuickedException after any other run"""
        total = self._lib.quicked_batch_hit_total(self._h)
        if total < 0:
            raise QuickedException(QUICKED_ERROR)
        found = np.zeros(self.n, dtype=np.int32)
        off = np.zeros(self.n + 1, dtype=np.int64)
        hits = np.zeros(total, dtype=HIT_DTYPE)
        st = self._lib.quicked_batch_hit_counts(self._h, found.ctypes.data, None)
        if st >= 0:
            st = self._lib.quicked_batch_hits(self._h, hits.ctypes.data, off.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return found, off, hits

    def run_panel(self, mode, panel, max_dist=None, matrix=False, sync=True):
        """quicked_batch_run_panel: every text of the batch against the panel, a list of bytes (the batch's own patterns are
        ignored).  mode: SEARCH_PREFIX / SEARCH_INFIX, optionally | SEARCH_IUPAC or | SEARCH_IUPAC_PATTERN (the members are the
        pattern side).  max_dist: None = no bound, one int for every member, or one bound per member.  matrix=True keeps
        every member's {score, text_end} for panel_matrix().  | PANEL_NO_INDELS: by mismatches only (no insertions or deletions),
        text_start = text_end - m; sync only.  Sync runs only."""
        panel = [bytes(p) for p in panel]
        k = len(panel)
        pool = np.frombuffer(b"".join(panel) + b"\0", dtype=np.uint8)
        plen = np.array([len(p) for p in panel], dtype=np.int32)
        poff = np.zeros(max(k, 1), dtype=np.int64)
        if k > 1:
            poff[1:k] = np.cumsum(plen[:-1], dtype=np.int64)
        mode = int(mode) | (PANEL_MATRIX if matrix else 0)
        if max_dist is None:
            max_dist = 2**31 - 1
        if np.ndim(max_dist) == 0:
            st = self._lib.quicked_batch_run_panel(self._h, mode, k, pool.ctypes.data, poff.ctypes.data, plen.ctypes.data, None, int(max_dist), 1 if sync else 0)
        else:
            md = np.ascontiguousarray(max_dist, dtype=np.int32)
            if md.shape != (k,):
                raise ValueError("max_dist: one bound per panel member")
            st = self._lib.quicked_batch_run_panel(self._h, mode, k, pool.ctypes.data, poff.ctypes.data, plen.ctypes.data, md.ctypes.data, 0, 1 if sync else 0)
        if sync and st not in (QUICKED_ERROR, QUICKED_UNIMPLEMENTED):
            # what panel_matrix() sizes its arrays with: the panel of the last run that got past the argument checks (a queued run
            # has no matrix, and the getters show the run before it until the fetch)
            self._panel_k = k
        return st

    def panel_results(self):
        """-> a structured array of PANEL_HIT_DTYPE, one entry per text, of the last panel run: the best member, its score and
        located stretch text[text_start:text_end], the runner-up and its score; -1 where there is none.  QuickedException after
        any other run"""
        out = np.zeros(self.n, dtype=PANEL_HIT_DTYPE)
        st = self._lib.quicked_batch_panel_results(self._h, out.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return out

    def panel_matrix(self):
        """-> (scores, text_ends), int32 [n, n_patterns], of the last panel run with matrix=True: every member's distance and
        end in every text, -1 / -1 where the member is beyond its bound (or the text is empty).  QuickedException otherwise"""
        k = getattr(self, "_panel_k", 0)
        sc = np.zeros((self.n, max(k, 1)), dtype=np.int32)
        te = np.zeros((self.n, max(k, 1)), dtype=np.int32)
        st = self._lib.quicked_batch_panel_matrix(self._h, sc.ctypes.data, te.ctypes.data) if k > 0 else QUICKED_ERROR
        if st < 0:
            raise QuickedException(st)
        return sc, te

    def run_panel_all(self, mode, panel, max_dist=None, max_hits=16, sync=True):
        """quicked_batch_run_panel_all: every occurrence of every panel member in every text, at most max_hits (1 .. 4096) stored
        per text, ordered by (pattern, text_end).  mode, panel and max_dist as in run_panel (no matrix flag); PANEL_CIGARS OR-ed into
        mode aligns every stored occurrence besides (panel_hit_cigars()); PANEL_TAILS (INFIX only) reports every text's 3' tail
        besides (panel_tails()); PANEL_HEADS reports every text's 5' head besides (panel_heads()).  sync=False needs
        configure_panel_queue() first and no PANEL_CIGARS; fetch() then brings the results.  PANEL_NO_INDELS: the occurrences by
        mismatches only (no insertions or deletions), text_start = text_end - m; sync only, and not beside the three bits above."""
        panel = [bytes(p) for p in panel]
        k = len(panel)
        pool = np.frombuffer(b"".join(panel) + b"\0", dtype=np.uint8)
        plen = np.array([len(p) for p in panel], dtype=np.int32)
        poff = np.zeros(max(k, 1), dtype=np.int64)
        if k > 1:
            poff[1:k] = np.cumsum(plen[:-1], dtype=np.int64)
        if max_dist is None:
            max_dist = 2**31 - 1
        if np.ndim(max_dist) == 0:
            return self._lib.quicked_batch_run_panel_all(self._h, int(mode), k, pool.ctypes.data, poff.ctypes.data, plen.ctypes.data, None, int(max_dist),
                                                         int(max_hits), 1 if sync else 0)
        md = np.ascontiguousarray(max_dist, dtype=np.int32)
        if md.shape != (k,):
            raise ValueError("max_dist: one bound per panel member")
        return self._lib.quicked_batch_run_panel_all(self._h, int(mode), k, pool.ctypes.data, poff.ctypes.data, plen.ctypes.data, md.ctypes.data, 0,
                                                     int(max_hits), 1 if sync else 0)

    def run_panel_scan(self, mode, panel, max_dist=None, max_hits=16, window=0, sync=True):
        """quicked_batch_run_panel_scan: run_panel_all's results, exactly, with every text cut into windows of `window` columns
        (0: the library's choice; else a multiple of 64) and a lane per window: for a few long texts.  INFIX only; mode's flags,
        panel, max_dist and max_hits as in run_panel_all (PANEL_CIGARS included).  Read through panel_hit_counts() / panel_hits() /
        panel_hit_cigars().  Sync runs only."""
        return self._run_panel_scan(self._lib.quicked_batch_run_panel_scan, mode, panel, max_dist, max_hits, window, sync)

    def run_panel_scan_no_indels(self, mode, panel, max_dist=None, max_hits=16, window=0, sync=True):
        """quicked_batch_run_panel_scan_no_indels: run_panel_all(mode | PANEL_NO_INDELS)'s results, exactly, with every text cut
        into windows of `window` columns (0: the library's choice; else a multiple of 64) and a lane per window: a panel by
        mismatches only against a few long texts.  INFIX only; PANEL_NO_INDELS in mode is accepted and means nothing more.  Read
        through panel_hit_counts() / panel_hits().  Sync runs only."""
        return self._run_panel_scan(self._lib.quicked_batch_run_panel_scan_no_indels, mode, panel, max_dist, max_hits, window, sync)

    def _run_panel_scan(self, entry, mode, panel, max_dist, max_hits, window, sync):
        panel = [bytes(p) for p in panel]
        k = len(panel)
        pool = np.frombuffer(b"".join(panel) + b"\0", dtype=np.uint8)
        plen = np.array([len(p) for p in panel], dtype=np.int32)
        poff = np.zeros(max(k, 1), dtype=np.int64)
        if k > 1:
            poff[1:k] = np.cumsum(plen[:-1], dtype=np.int64)
        md, md_all = None, 2**31 - 1 if max_dist is None else max_dist
        if np.ndim(md_all) != 0:
            md, md_all = np.ascontiguousarray(max_dist, dtype=np.int32), 0
            if md.shape != (k,):
                raise ValueError("max_dist: one bound per panel member")
        return entry(self._h, int(mode), k, pool.ctypes.data, poff.ctypes.data, plen.ctypes.data,
                     None if md is None else md.ctypes.data, int(md_all), int(max_hits), int(window), 1 if sync else 0)

    def panel_hit_counts(self):
        """-> (found, stored) int32 arrays of the last all-occurrences panel run: found[i] occurrences of all members in text i
        (exact whatever the cap), stored[i] = min(found[i], max_hits).  QuickedException after any other run"""
        found = np.zeros(self.n, dtype=np.int32)
        stored = np.zeros(self.n, dtype=np.int32)
        st = self._lib.quicked_batch_panel_hit_counts(self._h, found.ctypes.data, stored.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return found, stored

    def panel_hits(self):
        """-> (hit_off, hits) of the last all-occurrences panel run: the stored occurrences of text i are
        hits[hit_off[i]:hit_off[i + 1]], a structured array of PANEL_OCC_DTYPE ordered by (pattern, text_end).
        QuickedException after any other run"""
        total = self._lib.quicked_batch_panel_hit_total(self._h)
        if total < 0:
            raise QuickedException(QUICKED_ERROR)
        off = np.zeros(self.n + 1, dtype=np.int64)
        hits = np.zeros(total, dtype=PANEL_OCC_DTYPE)
        st = self._lib.quicked_batch_panel_hits(self._h, hits.ctypes.data, off.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return off, hits

    def configure_panel_tails(self, min_overlap=3):
        """quicked_batch_configure_panel_tails: the shortest tail (1 .. PANEL_MAX_LEN) of the PANEL_TAILS runs to come.  -> the
        status"""
        return self._lib.quicked_batch_configure_panel_tails(self._h, min_overlap)

    def panel_tails(self):
        """-> a structured array of PANEL_TAIL_DTYPE, one per text, of the last run_panel_all whose mode had PANEL_TAILS: the
        panel member cut off by the text's end -- its first `overlap` bases fit text[text_start:] at distance `score` --, every
        field -1 where no member has a tail.  QuickedException after any other run"""
        out = np.zeros(max(self.n, 1), dtype=PANEL_TAIL_DTYPE)
        st = self._lib.quicked_batch_panel_tails(self._h, out.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return out[:self.n]

    def configure_panel_queue(self, max_total):
        """quicked_batch_configure_panel_queue: 0 (the default) keeps run_panel / run_panel_all sync only; 1 .. 2**26 lets this
        batch object queue them (sync=False) and is the room for the records of a queued run_panel_all.  -> the status"""
        return self._lib.quicked_batch_configure_panel_queue(self._h, int(max_total))

    def panel_queue_wanted(self):
        """-> the total a fetched queued run_panel_all would have stored without max_total (above it: the records are the first
        max_total of them), -1 after anything else"""
        return int(self._lib.quicked_batch_panel_queue_wanted(self._h))

    def configure_panel_heads(self, min_overlap=3):
        """quicked_batch_configure_panel_heads: the shortest head (1 .. PANEL_MAX_LEN) of the PANEL_HEADS runs to come; the tails'
        setting is its own.  -> the status"""
        return self._lib.quicked_batch_configure_panel_heads(self._h, min_overlap)

    def panel_heads(self):
        """-> a structured array of PANEL_HEAD_DTYPE, one per text, of the last run_panel_all whose mode had PANEL_HEADS: the
        panel member cut off by the text's start -- its last `overlap` bases fit text[:text_end] at distance `score` --, every
        field -1 where no member has a head.  QuickedException after any other run"""
        out = np.zeros(max(self.n, 1), dtype=PANEL_HEAD_DTYPE)
        st = self._lib.quicked_batch_panel_heads(self._h, out.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return out[:self.n]

    def panel_hit_cigars(self):
        """-> [str], one per stored occurrence in panel_hits() order, of the last run_panel_all / run_panel_scan whose mode had
        PANEL_CIGARS: the global alignment of the occurrence's member against text[text_start:text_end] in the batch's
        cigar_style (None where the run reported a disagreement).  QuickedException after any other run"""
        nbytes = self._lib.quicked_batch_panel_hit_cigar_bytes(self._h)
        total = self._lib.quicked_batch_panel_hit_total(self._h)
        if nbytes < 0 or total < 0:
            raise QuickedException(QUICKED_ERROR)
        pool = np.zeros(max(int(nbytes), 1), dtype=np.uint8)
        off = np.zeros(max(int(total), 1), dtype=np.int64)
        st = self._lib.quicked_batch_panel_hit_cigars(self._h, pool.ctypes.data, off.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        raw = pool.tobytes()
        return [None if o < 0 else raw[o:raw.index(b"\0", o)].decode() for o in off[:total].tolist()]

    def locations(self):
        """-> (text_start, text_end) int32 arrays of the last search run: the located stretch is text[start:end]; -1 / -1 for a
        pair beyond its bound or with an empty sequence.  QuickedException after a run that was not a search run"""
        ts = np.zeros(self.n, dtype=np.int32)
        te = np.zeros(self.n, dtype=np.int32)
        st = self._lib.quicked_batch_locations(self._h, ts.ctypes.data, te.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return ts, te

    def sync(self):
        return self._lib.quicked_batch_sync(self._h)

    def fetch(self):
        """results of the last sync=False run -> host (quicked_batch_fetch)"""
        return self._lib.quicked_batch_fetch(self._h)

    def reload(self, batch):
        """new pairs into the same batch object (quicked_batch_reload): the device arena is reused"""
        self._keep = batch
        self.n = len(batch)
        return self._lib.quicked_batch_reload(
            self._h, self.n, batch.pattern_pool.ctypes.data, batch.pattern_off.ctypes.data, batch.pattern_len.ctypes.data,
            batch.text_pool.ctypes.data, batch.text_off.ctypes.data, batch.text_len.ctypes.data)

    def reload_wire(self, batch, wire, pw, po, tw, to):
        self._keep = (batch, pw, po, tw, to)
        self.n = len(batch)
        return self._lib.quicked_batch_reload_packed(
            self._h, self.n, wire, pw.ctypes.data, po.ctypes.data, batch.pattern_len.ctypes.data,
            tw.ctypes.data, to.ctypes.data, batch.text_len.ctypes.data)

    def configure(self, cigar_style=0, check=False):
        """cigar_style 0 = reference RLE "MXID", 1 = SAM "=XID", 2 = SAM "MID"; check = device-side validator"""
        return self._lib.quicked_batch_configure(self._h, cigar_style, 1 if check else 0)

    def configure_tags(self, stats=False, md=False, cigar=True):
        """quicked_batch_configure_tags for the sync runs to come: stats = a row of pair_stats() per pair, md = the SAM MD:Z
        strings, cigar=False = align but format and download no CIGAR strings.  -> the status (QUICKED_UNIMPLEMENTED: md on a
        packed batch)"""
        return self._lib.quicked_batch_configure_tags(
            self._h, (TAG_STATS if stats else 0) | (TAG_MD if md else 0) | (0 if cigar else TAG_NO_CIGAR))

    def pair_stats(self):
        """-> (n, 8) int32: matches, mismatches, ins_bases, del_bases, ins_runs, del_runs, longest_match, columns per pair (all
        -1: no alignment).  QuickedException after a run that produced none"""
        out = np.zeros((self.n, 8), dtype=np.int32)
        st = self._lib.quicked_batch_pair_stats(self._h, out.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return out

    def md(self):
        """-> one MD:Z string (or None) per pair; the pattern is SAM's reference.  QuickedException after a run that produced none"""
        nb = self._lib.quicked_batch_md_bytes(self._h)
        pool = np.zeros(max(nb, 1), dtype=np.uint8)
        off = np.zeros(self.n, dtype=np.int64)
        st = self._lib.quicked_batch_md(self._h, pool.ctypes.data, off.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        raw = pool.tobytes()
        return [None if o < 0 else raw[o:raw.index(b"\0", o)].decode("latin-1") for o in off]

    def validate(self, cigars):
        """device-side cigar_check_alignment of one CIGAR string (or None) per pair -> int32 verdicts"""
        off = np.full(self.n, -1, dtype=np.int64)
        blob = bytearray()
        for i, c in enumerate(cigars):
            if c is not None:
                off[i] = len(blob)
                blob += c.encode() + b"\0"
        ok = np.zeros(self.n, dtype=np.int32)
        st = self._lib.quicked_batch_validate(self._h, bytes(blob), len(blob), off.ctypes.data, ok.ctypes.data)
        if st < 0:
            raise QuickedException(st)
        return ok

    def check_results(self):
        ok = np.zeros(self.n, dtype=np.int32)
        self._lib.quicked_batch_check_results(self._h, ok.ctypes.data)
        return ok

    def scores(self):
        s = np.zeros(self.n, dtype=np.int32)
        st = np.zeros(self.n, dtype=np.int32)
        self._lib.quicked_batch_scores(self._h, s.ctypes.data, st.ctypes.data)
        return s, st

    def cigars(self):
        nb = self._lib.quicked_batch_cigar_bytes(self._h)
        pool = np.zeros(max(nb, 1), dtype=np.uint8)
        off = np.zeros(self.n, dtype=np.int64)
        self._lib.quicked_batch_cigars(self._h, pool.ctypes.data, off.ctypes.data)
        raw = pool.tobytes()
        out = []
        for o in off:
            if o < 0:
                out.append(None)
            else:
                e = raw.index(b"\0", o)
                out.append(raw[o:e].decode())
        return out

    def cigar_view(self):
        """-> (uint8 view of the batch's pinned string pool, int64 view of the per-pair offsets), no copies; valid until
        the next synchronous run / fetch / reload of the batch"""
        pool, off = C.c_void_p(), C.c_void_p()
        st = self._lib.quicked_batch_cigar_view(self._h, C.byref(pool), C.byref(off))
        if st < 0:
            raise QuickedException(st)
        nb = self._lib.quicked_batch_cigar_bytes(self._h)
        pv = np.ctypeslib.as_array((C.c_uint8 * max(nb, 1)).from_address(pool.value))[:nb] if (nb and pool.value) else np.zeros(0, np.uint8)
        ov = np.ctypeslib.as_array((C.c_int64 * self.n).from_address(off.value)) if self.n else np.zeros(0, np.int64)
        return pv, ov

    def deferred_pairs(self):
        """pairs of the last fetched / synchronous QuickEd run that were aligned at fetch time (quicked_batch.h)"""
        return int(self._lib.quicked_batch_deferred_pairs(self._h))

    def counters(self):
        c = np.zeros(8, dtype=np.int64)
        self._lib.quicked_batch_counters(self._h, c.ctypes.data)
        return c

    def kernel_time(self):
        """-> (sum of dominant-kernel HIP-event ms, launches) since the last call"""
        ms, n = C.c_double(0), C.c_int64(0)
        self._lib.quicked_batch_kernel_time(self._h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def kernel_times(self):
        """-> (ms[4], launches[4]) by kind since the last call: 0 score-only passes, 1 fills, 2 Hirschberg half passes, 3 diagonal-word
        launches of bounded runs"""
        ms, n = np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.int64)
        self._lib.quicked_batch_kernel_times(self._h, ms.ctypes.data, n.ctypes.data)
        return ms, n

    def close(self):
        if self._h:
            self._lib.quicked_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def pinned_copy(batch):
    """The same pairs with the two byte pools in pinned host memory (quicked_host_alloc)."""
    import numpy as _np
    L = lib()
    out = []
    for pool in (batch.pattern_pool, batch.text_pool):
        ptr = L.quicked_host_alloc(max(pool.nbytes, 1))
        if not ptr:
            raise MemoryError("quicked_host_alloc failed")
        arr = _np.ctypeslib.as_array((C.c_uint8 * max(pool.nbytes, 1)).from_address(ptr))
        arr[:pool.nbytes] = pool
        out.append((arr, ptr))
    from .datagen import PairBatch
    pb = PairBatch(out[0][0], batch.pattern_off, batch.pattern_len, out[1][0], batch.text_off, batch.text_len)
    pb._pinned = [p for _, p in out]
    return pb


def pinned_array(arr):
    """a copy of a numpy array in pinned host memory -> (array, pointer for quicked_host_free)"""
    import numpy as _np
    L = lib()
    ptr = L.quicked_host_alloc(max(arr.nbytes, 8))
    if not ptr:
        raise MemoryError("quicked_host_alloc failed")
    out = _np.ctypeslib.as_array((C.c_uint8 * max(arr.nbytes, 8)).from_address(ptr))[:arr.nbytes].view(arr.dtype)
    out[:] = arr
    return out, ptr


def pinned_free(pb):
    for p in getattr(pb, "_pinned", []):
        lib().quicked_host_free(p)
    pb._pinned = []
