"""ctypes binding of libandihip.so (include/andi_hip.h).

The names follow the reference's functions (seq_subject_init, esa_init,
get_match_cached, dist_anchor, distMatrix, estimate_*).  There is no CPU
fallback: if the library is missing or no HIP device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ANDI_HIP_LIB") or os.path.join(_HERE, "libandihip.so")  # override: diagnostic builds

M_RAW, M_JC, M_KIMURA, M_LOGDET, M_ANI = range(5)
MODEL_NAMES = {"raw": M_RAW, "jc": M_JC, "kimura": M_KIMURA, "logdet": M_LOGDET, "ani": M_ANI}


class AndiHipError(RuntimeError):
    pass


class Seq(C.Structure):
    _fields_ = [("seq", C.c_char_p), ("len", C.c_size_t)]


class Model(C.Structure):
    _fields_ = [("counts", C.c_uint32 * 16), ("seq_len", C.c_uint32)]


class Interval(C.Structure):
    _fields_ = [("l", C.c_int32), ("i", C.c_int32), ("j", C.c_int32), ("m", C.c_int32)]


PROGRESS_FN = C.CFUNCTYPE(None, C.c_size_t, C.c_size_t, C.c_void_p)


class Opts(C.Structure):
    _fields_ = [
        ("p_value", C.c_double),
        ("model", C.c_int),
        ("device", C.c_int),
        ("host_threads", C.c_int),
        ("low_memory", C.c_int),
        ("segment", C.c_uint32),
        ("progress", PROGRESS_FN),
        ("ud", C.c_void_p),
        ("sa_on_host", C.c_int),
        ("num_gpus", C.c_int),
        ("devices", C.POINTER(C.c_int)),
    ]


class Timings(C.Structure):
    _fields_ = [
        ("build_ms", C.c_double),
        ("build_launches", C.c_uint64),
        ("scan_ms", C.c_double),
        ("scan_launches", C.c_uint64),
        ("stitch_ms", C.c_double),
        ("stitch_launches", C.c_uint64),
        ("scan_query_nt", C.c_uint64),
        ("scan_pairs", C.c_uint64),
        ("fixups", C.c_uint64),
        ("reference_subjects", C.c_uint64),
        ("sa_ms", C.c_double),
        ("sa_builds", C.c_uint64),
        ("sa_rounds", C.c_uint64),
        ("adaptive_calls", C.c_uint64),
        ("uniform_calls", C.c_uint64),
        ("coop_calls", C.c_uint64),
        ("coop_fallbacks", C.c_uint64),
        ("routed_calls", C.c_uint64),
        ("coop_query_nt", C.c_uint64),
        ("lane_query_nt", C.c_uint64),
        ("pool_calls", C.c_uint64),
    ]


# every symbol include/andi_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "andi_hip_default_opts": (None, [C.POINTER(Opts)]),
    "andi_hip_abi_version": (C.c_int, []),
    "andi_hip_trim": (C.c_size_t, []),
    "andi_hip_pack_symbols": (C.c_int, [C.c_char_p, C.c_size_t, C.c_void_p]),
    "andi_hip_dist_matrix": (C.c_int, [_P, C.POINTER(Seq), C.c_size_t, C.POINTER(Opts), C.c_char_p, C.c_size_t]),
    "andi_hip_dist_rect": (C.c_int, [_P, _P, C.POINTER(Seq), C.c_size_t, C.POINTER(Seq), C.c_size_t, C.POINTER(Opts),
                                     C.c_char_p, C.c_size_t]),
    "andi_hip_last_gather": (C.c_char_p, []),
    "andi_hip_row_block": (None, [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "andi_hip_copy_ceiling": (C.c_int, [_P, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "andi_hip_subject_prepare": (C.c_int, [C.c_char_p, C.c_size_t, C.c_double, C.POINTER(_P),
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_double),
                                            C.POINTER(C.c_size_t)]),
    "andi_hip_free": (None, [_P]),
    "andi_hip_min_anchor_length": (C.c_size_t, [C.c_double, C.c_double, C.c_size_t]),
    "andi_hip_shustring_cum_prob": (C.c_double, [C.c_size_t, C.c_double, C.c_size_t]),
    "andi_hip_suffix_array": (C.c_int, [_P, _P, C.c_int32]),
    "andi_hip_suffix_sorter": (C.c_char_p, []),
    "andi_hip_model_average": (Model, [C.POINTER(Model), C.POINTER(Model)]),
    "andi_hip_model_coverage": (C.c_double, [C.POINTER(Model)]),
    "andi_hip_estimate": (C.c_double, [C.POINTER(Model), C.c_int]),
    "andi_hip_format_distances": (C.c_size_t, [_P, C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.c_int,
                                               C.c_int, C.c_int, _P, C.c_size_t, _P, C.c_size_t,
                                               C.POINTER(C.c_int)]),
    "andi_hip_format_distances_rect": (C.c_size_t, [_P, _P, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(C.c_char_p),
                                                    C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P,
                                                    C.c_size_t, C.POINTER(C.c_int)]),
    "andi_hip_distances": (C.c_int, [_P, C.c_size_t, C.c_int, _P]),
    "andi_hip_format_newick": (C.c_size_t, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, _P, C.c_size_t]),
    "andi_hip_format_newick_support": (C.c_size_t, [_P, _P, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, _P, C.c_size_t]),
    "andi_hip_format_newick_transfer": (C.c_size_t, [_P, _P, _P, C.c_size_t, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, _P,
                                                     C.c_size_t]),
    "andi_hip_consensus": (C.c_int, [_P, C.c_size_t, C.c_size_t, _P, _P, C.c_size_t, _P, _P, _P, C.POINTER(C.c_size_t)]),
    "andi_hip_format_newick_consensus": (C.c_size_t, [_P, C.c_size_t, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, _P,
                                                      C.c_size_t]),
    "andi_hip_nj": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "andi_hip_nj_batch": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P]),
    "andi_hip_tree": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "andi_hip_tree_batch": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_int, _P, _P]),
    "andi_hip_nj_support": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, _P]),
    "andi_hip_nj_splits": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, _P, _P, C.POINTER(C.c_size_t), C.POINTER(_P),
                                     C.POINTER(_P)]),
    "andi_hip_nj_transfer": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, _P]),
    "andi_hip_nj_transfer_taxa": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, C.c_double, _P, _P, _P, _P]),
    "andi_hip_linkage": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "andi_hip_linkage_batch": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_int, _P, _P]),
    "andi_hip_linkage_cut": (C.c_int, [_P, C.c_size_t, C.c_double, _P, C.POINTER(C.c_size_t)]),
    "andi_hip_cluster_medoids": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P]),
    "andi_hip_cluster_stability": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t, _P]),
    "andi_hip_format_newick_linkage": (C.c_size_t, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, _P, C.c_size_t]),
    "andi_hip_complete": (C.c_int, [_P, _P, C.c_size_t, C.c_uint, _P, _P, C.c_size_t, C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_size_t)]),
    "andi_hip_complete_batch": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_uint, _P, _P, _P]),
    "andi_hip_delta_scores": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "andi_hip_place": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.c_int, _P, _P, _P, _P]),
    "andi_hip_distances_rect": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.c_int, _P]),
    "andi_hip_root": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, _P]),
    "andi_hip_format_newick_rooted": (C.c_size_t, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, C.c_int32, C.c_double,
                                                   C.POINTER(C.c_char_p), _P, C.c_size_t]),
    "andi_hip_fit": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int, _P, _P, _P, _P]),
    "andi_hip_relength": (C.c_int, [_P, C.c_size_t, _P, _P]),
    "andi_hip_refine": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int, C.c_double, C.c_size_t, _P, _P, _P]),
    "andi_hip_refine_spr": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_double, C.c_size_t, _P, _P, _P]),
    "andi_hip_parse_newick": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), C.c_size_t, C.c_int, _P, C.c_char_p, C.c_size_t]),
    "andi_hip_format_jplace": (C.c_size_t, [_P, C.c_size_t, C.POINTER(C.c_char_p), C.c_int, _P, C.c_size_t,
                                            C.POINTER(C.c_char_p), C.c_int, _P, C.c_size_t]),
    "andi_hip_sketch": (C.c_int, [_P, C.POINTER(Seq), C.c_size_t, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "andi_hip_sketch_count": (C.c_size_t, [_P]),
    "andi_hip_sketch_sizes": (C.c_int, [_P, _P, _P]),
    "andi_hip_sketch_download": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "andi_hip_sketch_free": (None, [_P, _P]),
    "andi_hip_sketch_timings": (C.c_int, [_P, _P]),
    "andi_hip_sketch_shared": (C.c_int, [_P, _P, _P, _P]),
    "andi_hip_screen_select": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, _P, _P]),
    "andi_hip_screen": (C.c_int, [C.POINTER(Seq), C.c_size_t, C.POINTER(Seq), C.c_size_t, C.c_int, C.c_uint64, C.c_int, _P, _P, _P,
                                  C.c_char_p, C.c_size_t]),
    "andi_hip_device_count": (C.c_int, []),
    "andi_hip_reload_knobs": (None, []),
    "andi_hip_ctx_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_size_t]),
    "andi_hip_ctx_destroy": (None, [_P]),
    "andi_hip_ctx_expect_queries": (None, [_P, C.c_size_t]),
    "andi_hip_last_error": (C.c_char_p, [_P]),
    "andi_hip_sync": (C.c_int, [_P]),
    "andi_hip_esa_stage": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "andi_hip_esa_stage_text": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "andi_hip_esa_download_sa": (C.c_int, [_P, _P, _P]),
    "andi_hip_esa_build": (C.c_int, [_P, _P]),
    "andi_hip_esa_build_index": (C.c_int, [_P, _P]),
    "andi_hip_esa_build_index_batch": (C.c_int, [_P, C.POINTER(_P), C.c_size_t]),
    "andi_hip_esa_flags": (C.c_int, [_P, _P, _P]),
    "andi_hip_esa_download": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "andi_hip_esa_download_index": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int)]),
    "andi_hip_esa_single_form": (C.c_int, [_P]),
    "andi_hip_esa_free": (None, [_P, _P]),
    "andi_hip_esa_bytes": (C.c_size_t, [_P]),
    "andi_hip_queries_stage": (C.c_int, [_P, C.POINTER(Seq), C.c_size_t, C.POINTER(_P)]),
    "andi_hip_queries_free": (None, [_P, _P]),
    "andi_hip_queries_view": (C.c_int, [_P, _P, C.c_size_t, C.c_size_t, C.POINTER(_P)]),
    "andi_hip_match_positions": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, _P]),
    "andi_hip_scan_rows": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64), C.c_size_t, _P, C.c_int,
                                     C.c_uint32, _P]),
    "andi_hip_bootstrap": (C.c_int, [_P, _P, C.c_size_t, C.c_uint64, C.c_size_t, _P]),
    "andi_hip_bootstrap_range": (C.c_int, [_P, _P, C.c_size_t, C.c_uint64, C.c_size_t, C.c_size_t, _P]),
    "andi_hip_bootstrap_nj": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_size_t, C.c_size_t, _P, _P, _P]),
    "andi_hip_bootstrap_tree": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int, C.c_uint64, C.c_size_t, C.c_size_t, _P, _P,
                                          _P]),
    "andi_hip_estimate_portable": (C.c_int, [_P, C.c_size_t, C.c_int, _P]),
    "andi_hip_dev_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "andi_hip_dev_free": (None, [_P, _P]),
    "andi_hip_copy_to_host": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "andi_hip_timings_get": (C.c_int, [_P, C.POINTER(Timings)]),
    "andi_hip_timings_reset": (None, [_P]),
}

# test hooks only the suite's library exports (andi_amd/csrc/api.hip, -DANDI_TEST_HOOKS): set up where the library has them
HOOK_SYMBOLS = {
    "andi_hip_test_download_text": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, C.c_size_t]),
    "andi_hip_test_pack_text": (C.c_int, [_P, _P, C.c_int]),
    "andi_hip_test_coop_items": (C.c_int, [_P, _P, C.c_size_t, _P, _P, C.c_size_t, _P]),
    "andi_hip_test_call_edges": (C.c_int, [_P, _P, _P]),
    "andi_hip_test_pair_layout": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "andi_hip_test_query_codes": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "andi_hip_test_stitch_slots": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P, _P]),
    "andi_hip_test_layout_kernels": (C.c_int, [_P] * 22),
}

_lib = None


def load():
    """Load libandihip.so; raises AndiHipError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AndiHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C andi_amd/csrc); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in HOOK_SYMBOLS.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        _lib = L
        import atexit
        atexit.register(L.andi_hip_trim)  # the arena's retained chunks go back before the interpreter is torn down
    return _lib


def _seq_array(seqs):
    arr = (Seq * len(seqs))()
    for k, s in enumerate(seqs):
        arr[k].seq = s
        arr[k].len = len(s)
    return arr


# ---------------------------------------------------------------- host pieces
def subject_prepare(seq: bytes, p_value=0.025):
    """seq_subject_init (src/sequence.c:210): returns (RS, gc, threshold)."""
    L = load()
    rs, n, gc, thr = _P(), C.c_size_t(), C.c_double(), C.c_size_t()
    if L.andi_hip_subject_prepare(seq, len(seq), p_value, C.byref(rs), C.byref(n), C.byref(gc), C.byref(thr)):
        raise AndiHipError("andi_hip_subject_prepare failed")
    try:
        RS = C.string_at(rs, n.value)
    finally:
        L.andi_hip_free(rs)
    return RS, gc.value, thr.value


def min_anchor_length(p, g, l):
    return load().andi_hip_min_anchor_length(p, g, l)


def shustring_cum_prob(x, p, l):
    return load().andi_hip_shustring_cum_prob(x, p, l)


def suffix_array(text: bytes):
    """divsufsort stand-in (src/esa.c:303)."""
    n = len(text)
    buf = C.create_string_buffer(text, n + 1)
    sa = np.empty(n, dtype=np.int32)
    if load().andi_hip_suffix_array(C.cast(buf, _P), sa.ctypes.data, n):
        raise AndiHipError("andi_hip_suffix_array failed")
    return sa


def _model(counts17):
    m = Model()
    for k in range(16):
        m.counts[k] = int(counts17[k])
    m.seq_len = int(counts17[16])
    return m


def estimate(counts17, model=M_JC):
    return load().andi_hip_estimate(C.byref(_model(counts17)), model)


def coverage(counts17):
    return load().andi_hip_model_coverage(C.byref(_model(counts17)))


def format_distances(M, names, model=M_JC, extra_verbose=False, truncate_names=False, warnings=True):
    """print_distances (src/io.c:246): returns (phylip_text, warning_text, flags)."""
    L = load()
    M = np.ascontiguousarray(M, dtype=np.uint32)
    n = M.shape[0]
    assert M.shape == (n, n, 17)
    cnames = (C.c_char_p * n)(*[s.encode() if isinstance(s, str) else s for s in names])
    cap = 64 + n * (64 + 16 * n)
    warn = C.create_string_buffer(1 << 20)
    flags = C.c_int()
    for _ in range(2):  # the call returns the bytes it needs: long names get a second, exact buffer
        out = C.create_string_buffer(cap)
        need = L.andi_hip_format_distances(M.ctypes.data, cnames, n, model, int(extra_verbose), int(truncate_names),
                                           int(warnings), C.cast(out, _P), cap, C.cast(warn, _P), len(warn),
                                           C.byref(flags))
        if need < cap:
            break
        cap = need + 1
    return out.value.decode(), warn.value.decode(), flags.value


def _names(names):
    return (C.c_char_p * len(names))(*[s.encode() if isinstance(s, str) else s for s in names])


def format_distances_rect(MRQ, MQR, ref_names, query_names, model=M_JC, extra_verbose=False, truncate_names=False,
                          warnings=True):
    """The query-versus-reference table of dist_rect's (MRQ, MQR): returns (text, warning_text, flags)."""
    L = load()
    MRQ = np.ascontiguousarray(MRQ, dtype=np.uint32)
    MQR = np.ascontiguousarray(MQR, dtype=np.uint32)
    nr, nq = MRQ.shape[0], MQR.shape[0]
    assert MRQ.shape == (nr, nq, 17) and MQR.shape == (nq, nr, 17)
    assert len(ref_names) == nr and len(query_names) == nq
    rn, qn = _names(ref_names), _names(query_names)
    cap = 64 + 16 * nr + nq * (64 + 16 * nr) + sum(len(x) for x in ref_names) + sum(len(x) for x in query_names)
    warn = C.create_string_buffer(1 << 20)
    flags = C.c_int()
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        need = L.andi_hip_format_distances_rect(MRQ.ctypes.data, MQR.ctypes.data, rn, nr, qn, nq, model,
                                                int(extra_verbose), int(truncate_names), int(warnings),
                                                C.cast(out, _P), cap, C.cast(warn, _P), len(warn), C.byref(flags))
        if need < cap:
            break
        cap = need + 1
    return out.value.decode(), warn.value.decode(), flags.value


# andi_hip_nj_join: a record of a neighbor-joining tree (ids a, b, c -- c = -1 but in the final record -- and branch lengths)
NJ_JOIN = np.dtype([("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("pad", "<i4"), ("la", "<f8"), ("lb", "<f8"),
                    ("lc", "<f8")])


def distances(M, model=M_JC):
    """The (n, n) float64 distances format_distances prints (model_average of both directions; diagonal +0.0)."""
    M = np.ascontiguousarray(M, dtype=np.uint32)
    n = M.shape[0]
    assert M.shape == (n, n, 17)
    D = np.empty((n, n), np.float64)
    if load().andi_hip_distances(M.ctypes.data, n, model, D.ctypes.data):
        raise AndiHipError("andi_hip_distances failed")
    return D


def newick(joins, names, truncate_names=False, support=None):
    """The Newick line (ending in ";\n") of nj's records for the leaves `names`; with support (nj_support's counts, one
    per pair record) each count is the label of its internal node."""
    J = np.ascontiguousarray(joins, dtype=NJ_JOIN)
    n = len(names)
    cn = _names(names)
    cap = 64 + 40 * n + sum(len(x) for x in names)
    if support is not None:
        support = np.ascontiguousarray(support, dtype=np.uint32)
        assert len(support) >= max(n - 3, 0)
        cap += 10 * n
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        if support is None:
            need = load().andi_hip_format_newick(J.ctypes.data, n, cn, int(truncate_names), C.cast(out, _P), cap)
        else:
            need = load().andi_hip_format_newick_support(J.ctypes.data, support.ctypes.data, n, cn, int(truncate_names),
                                                         C.cast(out, _P), cap)
        if need < cap:
            break
        cap = need + 1
    return out.value.decode()


def newick_transfer(joins, depth, transfer, used, names, truncate_names=False):
    """The Newick line of nj's records with the transfer bootstrap expectation as the label of every inner branch
    (andi_hip_format_newick_transfer), from nj_transfer's depth and transfer summed over `used` replicates; "" where the
    library refuses (used == 0, a depth below 2, malformed records)."""
    J = np.ascontiguousarray(joins, dtype=NJ_JOIN)
    n = len(names)
    cn = _names(names)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    transfer = np.ascontiguousarray(transfer, dtype=np.uint64)
    assert len(depth) >= max(n - 3, 0) and len(transfer) >= max(n - 3, 0)
    cap = 64 + 56 * n + sum(len(x) for x in names)
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        need = load().andi_hip_format_newick_transfer(J.ctypes.data, depth.ctypes.data, transfer.ctypes.data, int(used), n, cn,
                                                      int(truncate_names), C.cast(out, _P), cap)
        if need < cap:
            break
        cap = need + 1
    return out.value.decode()


# andi_hip_cons_node: a node of a consensus tree (its parent's index, -1 for the root; the replicates that have its branch; its length)
CONS_NODE = np.dtype([("parent", "<i4"), ("support", "<u4"), ("length", "<f8")])


def _skip(skip, count):
    if skip is None:
        return None
    skip = np.ascontiguousarray(skip, dtype=np.uint8)
    assert skip.shape == (count,)
    return skip


def consensus(reps, ids, freq, sets, skip=None, n=None):
    """The majority-rule consensus tree (andi_hip_consensus) of the replicate trees reps (count, n - 2) from nj_splits'
    (ids, freq, sets): the nodes as a structured array of dtype CONS_NODE -- the n leaves, the majority splits in
    ascending id order, the root last.  n: the number of leaves, where one record per replicate leaves it open (2 or 3;
    by default 2 if the first replicate's record has no third child)."""
    reps = np.ascontiguousarray(reps, dtype=NJ_JOIN)
    assert reps.ndim == 2
    count = reps.shape[0]
    if n is None:
        n = 2 if reps.shape[1] == 1 and int(reps[0, 0]["c"]) < 0 else reps.shape[1] + 2
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    sets = np.ascontiguousarray(sets, dtype=np.uint64)
    assert ids.size == count * max(n - 3, 0) and sets.size == freq.size * ((n + 63) // 64)
    skip = _skip(skip, count)
    nodes = np.zeros(max(2 * n - 2, 3), CONS_NODE)
    m = C.c_size_t(0)
    if load().andi_hip_consensus(reps.ctypes.data, n, count, skip.ctypes.data if skip is not None else None,
                                 ids.ctypes.data, freq.size, freq.ctypes.data, sets.ctypes.data, nodes.ctypes.data,
                                 C.byref(m)):
        raise AndiHipError("andi_hip_consensus: inconsistent arguments")
    return nodes[:n + m.value + 1].copy()


def newick_consensus(nodes, names, truncate_names=False):
    """The Newick line (ending in ";\n") of consensus' nodes for the leaves `names`: every inner node labelled with the
    number of replicates that have its branch; "" for malformed nodes."""
    nodes = np.ascontiguousarray(nodes, dtype=CONS_NODE)
    n = len(names)
    ninner = len(nodes) - n - 1
    if ninner < 0:
        return ""
    cn = _names(names)
    cap = 64 + 60 * n + sum(len(x) for x in names)
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        need = load().andi_hip_format_newick_consensus(nodes.ctypes.data, n, ninner, cn, int(truncate_names),
                                                       C.cast(out, _P), cap)
        if need < cap:
            break
        cap = need + 1
    return out.value.decode()


# andi_hip_link: a record of a linkage tree (SciPy's Z: the two node ids, the leaves below the new node, its height)
LINK = np.dtype([("a", "<i4"), ("b", "<i4"), ("size", "<u4"), ("pad", "<u4"), ("height", "<f8")])
LINKAGE_METHODS = {"single": 0, "complete": 1, "average": 2}


def _method(method):
    if method not in LINKAGE_METHODS:
        raise ValueError("linkage method %r: expected single, complete or average" % (method,))
    return LINKAGE_METHODS[method]


def linkage_cut(Z, t):
    """Flat clusters of linkage's records at threshold t (andi_hip_linkage_cut): uint32[n] labels, 0-based, numbered by
    first appearance in ascending leaf id.  No GPU is touched."""
    Z = np.ascontiguousarray(Z, dtype=LINK)
    n = len(Z) + 1
    labels = np.zeros(n, np.uint32)
    k = C.c_size_t(0)
    if load().andi_hip_linkage_cut(Z.ctypes.data, n, float(t), labels.ctypes.data, C.byref(k)):
        raise AndiHipError("andi_hip_linkage_cut: malformed records")
    return labels


def cluster_medoids(D, labels):
    """One representative per cluster (andi_hip_cluster_medoids): uint32[nclusters], the member with the least summed
    distance to its cluster.  No GPU is touched."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    n = D.shape[0]
    assert D.shape == (n, n) and labels.shape == (n,)
    k = int(labels.max()) + 1
    medoid = np.zeros(k, np.uint32)
    if load().andi_hip_cluster_medoids(D.ctypes.data, n, labels.ctypes.data, k, medoid.ctypes.data):
        raise AndiHipError("andi_hip_cluster_medoids: bad arguments")
    return medoid


def cluster_stability(labels, rep_labels):
    """In how many of the replicates' clusterings rep_labels (count, n) every cluster of `labels` recurs exactly
    (andi_hip_cluster_stability): uint32[nclusters].  No GPU is touched."""
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    rep_labels = np.ascontiguousarray(rep_labels, dtype=np.uint32)
    n = len(labels)
    assert rep_labels.ndim == 2 and rep_labels.shape[1] == n
    k = int(labels.max()) + 1
    stability = np.zeros(k, np.uint32)
    if load().andi_hip_cluster_stability(labels.ctypes.data, k, rep_labels.ctypes.data, n, rep_labels.shape[0],
                                         stability.ctypes.data):
        raise AndiHipError("andi_hip_cluster_stability: bad arguments")
    return stability


def newick_linkage(Z, names, truncate_names=False):
    """The Newick line (ending in ";\n") of linkage's records for the leaves `names`, a rooted dendrogram; "" for malformed
    records and for a branch that is not finite (a height of +inf)."""
    Z = np.ascontiguousarray(Z, dtype=LINK)
    n = len(names)
    assert len(Z) == n - 1
    cn = _names(names)
    cap = 64 + 40 * n + sum(len(x) for x in names)
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        need = load().andi_hip_format_newick_linkage(Z.ctypes.data, n, cn, int(truncate_names), C.cast(out, _P), cap)
        if need < cap:
            break
        cap = need + 1
    return out.value.decode()


# andi_hip_placement: where a query sits on a tree (the edge, -1 for none; the usable leaves; the point on the edge from
# its child end; the length of the hanging branch; the weighted squared error)
PLACEMENT = np.dtype([("edge", "<i4"), ("used", "<u4"), ("distal", "<f8"), ("pendant", "<f8"), ("err", "<f8")])
PLACE_METHODS = {"ols": 0, "fm": 1}


def _place_method(method):
    if method not in PLACE_METHODS:
        raise ValueError("placement method %r: expected fm or ols" % (method,))
    return PLACE_METHODS[method]


def distances_rect(MRQ, MQR, model=M_JC):
    """The (nq, nr) float64 distances format_distances_rect prints for dist_rect's (MRQ, MQR), unrounded
    (andi_hip_distances_rect).  No GPU is touched."""
    MRQ = np.ascontiguousarray(MRQ, dtype=np.uint32)
    MQR = np.ascontiguousarray(MQR, dtype=np.uint32)
    nr, nq = MRQ.shape[0], MQR.shape[0]
    assert MRQ.shape == (nr, nq, 17) and MQR.shape == (nq, nr, 17)
    D = np.empty((nq, nr), np.float64)
    if load().andi_hip_distances_rect(MRQ.ctypes.data, MQR.ctypes.data, nr, nq, model, D.ctypes.data):
        raise AndiHipError("andi_hip_distances_rect failed")
    return D


def parse_newick(text, names, truncate_names=False):
    """The n - 2 records (dtype NJ_JOIN) of the unrooted binary tree in the Newick `text` whose leaves are `names`
    (andi_hip_parse_newick, the inverse of newick); AndiHipError with the parser's message, which names the byte offset,
    for a text it refuses.  No GPU is touched."""
    n = len(names)
    J = np.zeros(max(n - 2, 0), NJ_JOIN)
    err = C.create_string_buffer(512)
    raw = text.encode() if isinstance(text, str) else bytes(text)
    if load().andi_hip_parse_newick(raw, _names(names), n, int(truncate_names), J.ctypes.data, err, len(err)):
        raise AndiHipError(err.value.decode(errors="replace"))
    return J


def jplace(J, ref_names, placements, query_names, method="fm", truncate_names=False):
    """The jplace text (version 3) of place's records for the tree J over `ref_names` (andi_hip_format_jplace); "" where
    the library refuses (malformed records).  No GPU is touched."""
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    P = np.ascontiguousarray(placements, dtype=PLACEMENT)
    n, nq = len(ref_names), len(query_names)
    assert len(J) == n - 2 and P.shape == (nq,)
    rn, qn = _names(ref_names), _names(query_names)
    cap = 512 + 64 * n + sum(len(x) for x in ref_names) + 128 * nq + sum(len(x) for x in query_names)
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        need = load().andi_hip_format_jplace(J.ctypes.data, n, rn, int(truncate_names), P.ctypes.data, nq, qn,
                                             _place_method(method), C.cast(out, _P), cap)
        if need < cap:
            break
        cap = need + 1
    return out.value.decode()


# ---------------------------------------------------------------- device objects
class Context:
    def __init__(self, device=0):
        L = load()
        self._h = _P()
        err = C.create_string_buffer(512)
        if L.andi_hip_ctx_create(C.byref(self._h), device, err, len(err)):
            raise AndiHipError(err.value.decode())
        self.device = device

    def expect_queries(self, queries):
        """queries per subject from now on (decides the depth of the probe tables; results do not depend on it)"""
        load().andi_hip_ctx_expect_queries(self._h, int(queries))

    def _check(self, rc, what):
        if rc:
            raise AndiHipError(f"{what}: {load().andi_hip_last_error(self._h).decode()}")

    def sync(self):
        self._check(load().andi_hip_sync(self._h), "sync")

    def timings(self):
        t = Timings()
        self._check(load().andi_hip_timings_get(self._h, C.byref(t)), "timings")
        return {k: getattr(t, k) for k, _ in Timings._fields_}

    def timings_reset(self):
        load().andi_hip_timings_reset(self._h)

    def coop_items(self):
        """(a test hook) the last routed scan call's list of the wavefront kernel's segments: (items or None if the call had no
        list, the pairs' class bytes, their cost classes, segments per subject of that kernel's layout)"""
        hook = _hook("andi_hip_test_coop_items")
        info = np.zeros(4, np.uint32)
        self._check(hook(self._h, None, 0, None, None, 0, info.ctypes.data), "test_coop_items")
        items, cls, cost = np.zeros(int(info[0]), np.uint32), np.zeros(int(info[1]), np.uint8), np.zeros(int(info[1]), np.uint8)
        self._check(hook(self._h, items.ctypes.data, len(items), cls.ctypes.data, cost.ctypes.data, len(cls), info.ctypes.data), "test_coop_items")
        return (items if info[3] else None), cls, cost, int(info[2])

    def call_edges(self):
        """(a test hook) what the last routed scan call enqueued around pass A, per layout ("lanes", "coop", "back": the lane scan's, the
        wavefront kernel's, the pairs handed back): {layout: (pass A enqueued, rounds of stitching again enqueued)}, and the 16 counters of the
        wavefront kernel's layout as its pass B left them (scan.h: restitch_count -- [0 .. 2] stretches stitched again per round, [3] chains
        that left their segment on their own)"""
        out, count_b = np.zeros(8, np.uint32), np.zeros(16, np.uint32)
        self._check(_hook("andi_hip_test_call_edges")(self._h, out.ctypes.data, count_b.ctypes.data), "test_call_edges")
        edges = {name: (bool(out[k]), int(out[3 + k])) for k, name in enumerate(("lanes", "coop", "back"))}
        edges["ahead"], edges["again"] = bool(out[6]), bool(out[7])  # went ahead of the pending builds; ran again on a raised flag
        return edges, count_b

    def pair_layout(self):
        """(a test hook) the lane layout of the last routed scan call: dict of pair_waves, pair_wave0 (None where the lanes have one segment
        length), sub_order, and the layout's sixteen counters at the host's first look (None where the host did not look)"""
        hook = _hook("andi_hip_test_pair_layout")
        info = np.zeros(4, np.uint32)
        self._check(hook(self._h, None, None, None, None, info.ctypes.data), "test_pair_layout")
        pairs, nsub = int(info[0]), int(info[1])
        waves, wave0, order, counts = np.zeros(pairs, np.uint32), np.zeros(pairs + 1, np.uint32), np.zeros(nsub, np.uint32), np.zeros(16, np.uint32)
        self._check(hook(self._h, waves.ctypes.data, wave0.ctypes.data, order.ctypes.data, counts.ctypes.data, info.ctypes.data), "test_pair_layout")
        return {"pair_waves": waves, "pair_wave0": wave0 if info[2] else None, "sub_order": order, "counts": counts if info[3] else None}

    def layout_kernels(self, nsub, nq, qlen, self_q, pair_class, pair_waves, pair_cost=None, sub_cost=None, *, struct_waves=0, seg0=64, max_class=3,
                       route_seg=2048, route_all_few=0, adaptive=1, items_order=1, sub_order=True, listed=True, allow_small=True, left=None):
        """(a test hook) the layout kernels of a routed scan call alone, on the caller's arrays (api.hip: andi_hip_test_layout_kernels; no
        subject, no query text, no sampling): pair_class, pair_waves, pair_cost of all nsub * nq pairs and sub_cost as k_pair_estimate would
        leave them, struct_waves its restitch_count[ANDI_STRUCT_WAVES]; left: a mask of the pairs marked ANDI_ROUTE_LEFT behind the routing
        (None: no second layout).  Returns a dict: stage 1 -- pair_class, pair_waves, pair_wave0 (None unless adaptive), sub_order (None
        without one), counts, quad (k_lane_quad's list), items (None without a list) --, stage 2 -- pair_class2, route_nt and, with `left`,
        pair_waves2, pair_wave02 (adaptive), counts2 --, and path (1: one block, 2: several kernels), sort_launches, total_segs."""
        hook = _hook("andi_hip_test_layout_kernels")
        P, LIMIT = int(nsub) * int(nq), 1 << 27
        u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
        qlen, self_q = u32(qlen), np.ascontiguousarray(self_q, dtype=np.int64)
        pair_class, pair_waves = np.ascontiguousarray(pair_class, dtype=np.uint8), u32(pair_waves)
        pair_cost = None if pair_cost is None else np.ascontiguousarray(pair_cost, dtype=np.uint8)
        sub_cost = None if sub_cost is None else np.ascontiguousarray(sub_cost, dtype=np.float32)
        left = None if left is None else np.ascontiguousarray(np.asarray(left) != 0, dtype=np.uint8)
        sane = 0 < P <= LIMIT  # (beyond: the library refuses before it reads an array)
        if sane:
            for arr, n in ((qlen, nq), (self_q, nsub), (pair_class, P), (pair_waves, P), (pair_cost, P), (sub_cost, nsub), (left, P)):
                if arr is not None and arr.shape != (n,):
                    raise ValueError("layout_kernels: an array of %s where %d entries are due" % (arr.shape, n))
        par = np.array([nsub, nq, struct_waves, seg0, max_class, route_seg, route_all_few, adaptive, items_order, int(bool(sub_order)), int(bool(listed)),
                        int(bool(allow_small))], dtype=np.uint32)
        total = int(((qlen.astype(np.int64) + route_seg - 1) // route_seg).sum()) if sane and route_seg > 0 else 0
        quad_cap = int(pair_waves.sum(dtype=np.int64)) + int(nsub) * int((((qlen.astype(np.int64) + seg0 - 1) // seg0 + 63) // 64).sum()) if sane and seg0 > 0 else 0
        z = lambda n, t=np.uint32: np.zeros(n, t) if sane and n <= LIMIT else None
        out = {"pair_class": z(P, np.uint8), "pair_waves": z(P), "pair_wave0": z(P + 1) if adaptive else None, "sub_order": z(nsub) if sub_order else None,
               "counts": np.zeros(16, np.uint32), "quad": z(quad_cap), "items": z(int(nsub) * total) if listed else None, "pair_class2": z(P, np.uint8),
               "pair_waves2": z(P) if left is not None else None, "pair_wave02": z(P + 1) if left is not None and adaptive else None,
               "counts2": np.zeros(16, np.uint32) if left is not None else None, "route_nt": np.zeros(3, np.uint64)}
        info = np.zeros(4, np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        self._check(hook(self._h, p(par), p(qlen), p(self_q), p(pair_class), p(pair_waves), p(pair_cost), p(sub_cost), p(left),
                         *[p(out[k]) for k in ("pair_class", "pair_waves", "pair_wave0", "sub_order", "counts", "quad", "items", "pair_class2",
                                               "pair_waves2", "pair_wave02", "counts2", "route_nt")], p(info)), "test_layout_kernels")
        if out["quad"] is not None:
            out["quad"] = out["quad"][: int(out["counts"][13])]  # (scan.h: ANDI_QUAD_WAVES)
        if out["items"] is not None:
            out["items"] = out["items"][: int(out["counts"][7])]  # (ANDI_COOP_SEGS)
        out.update(path=int(info[0]), sort_launches=int(info[1]), total_segs=int(info[2]))
        return out

    def stitch_slots(self):
        """(a test hook) the per-slot records of the last scan call that used one segment length (not routed, no per-pair lengths),
        as passes A and B left them in the call's scratch: a dict of uint32 arrays -- cold_exit, true_exit, used_entry (slots, 8:
        p, lastS, lastQ, lastLen, lwra, pad[3]), cold_counts, owned (slots, 16), marks (slots, 28: the mark's state, its 16 counts,
        the first anchor's pos_Q, pos_S, length, 0), restitch_count (16) -- and nsub, total_segs, seg.  The slot of segment k of
        query q under subject s is s * total_segs + qseg_start[q] + k, qseg_start the running sum of ceil(qlen / seg)."""
        hook = _hook("andi_hip_test_stitch_slots")
        info = np.zeros(4, np.uint32)
        self._check(hook(self._h, None, None, None, None, None, None, 0, None, info.ctypes.data), "test_stitch_slots")
        if not info[3]:
            raise AndiHipError("test_stitch_slots: no scan call with one segment length on record")
        n = int(info[0]) * int(info[1])
        out = {"cold_exit": np.zeros((n, 8), np.uint32), "true_exit": np.zeros((n, 8), np.uint32), "used_entry": np.zeros((n, 8), np.uint32),
               "cold_counts": np.zeros((n, 16), np.uint32), "owned": np.zeros((n, 16), np.uint32), "marks": np.zeros((n, 28), np.uint32),
               "restitch_count": np.zeros(16, np.uint32)}
        p = {k: v.ctypes.data for k, v in out.items()}
        self._check(hook(self._h, p["cold_exit"], p["true_exit"], p["used_entry"], p["cold_counts"], p["owned"], p["marks"], n,
                         p["restitch_count"], info.ctypes.data), "test_stitch_slots")
        out.update(nsub=int(info[0]), total_segs=int(info[1]), seg=int(info[2]))
        return out

    def alloc(self, nbytes):
        p = _P()
        self._check(load().andi_hip_dev_alloc(self._h, nbytes, C.byref(p)), "dev_alloc")
        return p

    def free(self, p):
        load().andi_hip_dev_free(self._h, p)

    def close(self):
        if self._h:
            load().andi_hip_ctx_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Esa:
    """esa_s (src/esa.h:42) resident in HBM: host prepares RS + SA; the device
    builds the scan index (build="index", default) and/or the reference's own
    arrays LCP, CLD, FVC, 10-mer table (build="reference")."""

    def __init__(self, ctx: Context, seq: bytes, p_value=0.025, sa=None, build="index", prepared=None):
        """sa: None = suffix array by the host sorter; an int32 array = given; "device" = built on the device."""
        self.ctx = ctx
        if prepared is not None:  # (RS, gc, threshold, SA) from prepare_host(), e.g. made in a thread pool
            self.RS, self.gc, self.threshold, sa = prepared
        else:
            self.RS, self.gc, self.threshold = subject_prepare(seq, p_value)
        self.n = len(self.RS)
        self._h = _P()
        L = load()
        if isinstance(sa, str) and sa == "device":
            self._SA = None
            ctx._check(L.andi_hip_esa_stage_text(ctx._h, self.RS, self.n, self.threshold, C.byref(self._h)),
                       "esa_stage_text")
        else:
            self._SA = suffix_array(self.RS) if sa is None else np.ascontiguousarray(sa, dtype=np.int32)
            ctx._check(L.andi_hip_esa_stage(ctx._h, self.RS, self._SA.ctypes.data, self.n, self.threshold,
                                            C.byref(self._h)), "esa_stage")
        self.reference_built = False
        if build in ("index", "both", True):
            self.build()
        if build in ("reference", "both"):
            self.build_reference()

    @property
    def SA(self):
        if self._SA is None:  # built on the device: fetch it
            sa = np.empty(self.n, np.int32)
            self.ctx._check(load().andi_hip_esa_download_sa(self.ctx._h, self._h, sa.ctypes.data), "esa_download_sa")
            self._SA = sa
        return self._SA

    def build(self):
        """scan index (probe table)"""
        self.ctx._check(load().andi_hip_esa_build_index(self.ctx._h, self._h), "esa_build_index")

    def build_reference(self):
        """LCP, CLD, FVC, 10-mer table"""
        self.ctx._check(load().andi_hip_esa_build(self.ctx._h, self._h), "esa_build")
        self.reference_built = True

    def flags(self):
        out = np.zeros(4, np.int32)
        self.ctx._check(load().andi_hip_esa_flags(self.ctx._h, self._h, out.ctypes.data), "esa_flags")
        return out

    def download(self):
        if not self.reference_built:
            self.build_reference()
        n = self.n
        LCP = np.empty(n + 1, np.int32)
        CLD = np.empty(n + 1, np.int32)
        FVC = np.empty(n, np.uint8)
        cache = np.empty((1 << 20, 4), np.int32)
        self.ctx._check(load().andi_hip_esa_download(self.ctx._h, self._h, LCP.ctypes.data, CLD.ctypes.data,
                                                     FVC.ctypes.data, cache.ctypes.data), "esa_download")
        return LCP, CLD, FVC, cache

    def download_index(self):
        """(K, table): the probe table of the scan index, uint32[4^K, 2] (test hook; andi_hip.h has the layout)."""
        K = C.c_int(0)
        self.ctx._check(load().andi_hip_esa_download_index(self.ctx._h, self._h, None, C.byref(K)), "esa_download_index")
        table = np.empty((1 << (2 * K.value), 2), np.uint32)
        self.ctx._check(load().andi_hip_esa_download_index(self.ctx._h, self._h, table.ctypes.data, C.byref(K)),
                        "esa_download_index")
        return K.value, table

    def pack_text(self, forms=3):
        """test hook: the index build's pack kernel alone on the staged text (forms: bit 0 with N1, bit 1 with P)"""
        self.ctx._check(_hook("andi_hip_test_pack_text")(self.ctx._h, self._h, forms), "test_pack_text")

    def download_text(self, beyond=16):
        """(N0, N1, P): the text as the scan index keeps it (test hook) -- N0 and N1 as bytes: the n + 1 + 64 symbols
        rounded up to pairs of words, and `beyond` bytes more; P as words from the block of padding in front of it on
        (P proper starts at word 3): (n + 1 + 64 + 31) // 32 blocks of three, and beyond // 4 words more."""
        nib = (self.n + 1 + 64 + 15) // 16 * 8 + beyond
        N0, N1 = np.empty(nib, np.uint8), np.empty(nib, np.uint8)
        P = np.empty(3 + 3 * ((self.n + 1 + 64 + 31) // 32) + beyond // 4, np.uint32)
        self.ctx._check(_hook("andi_hip_test_download_text")(self.ctx._h, self._h, N0.ctypes.data, N1.ctypes.data, nib,
                                                             P.ctypes.data, len(P)), "test_download_text")
        return N0, N1, P

    def single_form(self):
        """form of the probe table's entries of K-mers that occur once: 0 plain, 1 extended, 2 short extended"""
        return load().andi_hip_esa_single_form(self._h)

    def nbytes(self):
        return load().andi_hip_esa_bytes(self._h)

    def close(self):
        if self._h and self.ctx._h:
            load().andi_hip_esa_free(self.ctx._h, self._h)
        self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prepare_host(seq: bytes, p_value=0.025):
    """The host part of esa_init for one subject: RS, gc, threshold and the suffix
    array.  ctypes releases the GIL, so a ThreadPool runs these in parallel (the
    role of the OpenMP subject loop, src/dist_hack.h:46-52)."""
    RS, gc, thr = subject_prepare(seq, p_value)
    return RS, gc, thr, suffix_array(RS)


class Queries:
    def __init__(self, ctx: Context, seqs):
        self.ctx = ctx
        self.seqs = [bytes(s) for s in seqs]
        self._arr = _seq_array(self.seqs)
        self._h = _P()
        ctx._check(load().andi_hip_queries_stage(ctx._h, self._arr, len(self.seqs), C.byref(self._h)),
                   "queries_stage")

    def __len__(self):
        return len(self.seqs)

    def view(self, first, count):
        """queries [first, first + count) of this set on its device buffers (nothing copied): scan with it like any
        staged set; close it before this one"""
        return QueriesView(self, first, count)

    def codes(self, qidx):
        """(a test hook) the staged 2-bit codes of query qidx: two uint32 words per block of 32 symbols, over the whole of the
        query's place in the pool (its symbols, the NUL behind them and the padding up to the next multiple of 256)"""
        out = np.zeros(2 * ((len(self.seqs[qidx]) + 1 + 255) // 256 * 8), np.uint32)
        self.ctx._check(_hook("andi_hip_test_query_codes")(self.ctx._h, self._h, int(qidx), out.ctypes.data, len(out)), "test_query_codes")
        return out

    def close(self):
        if self._h and self.ctx._h:
            load().andi_hip_queries_free(self.ctx._h, self._h)
        self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QueriesView(Queries):
    """andi_hip_queries_view: a column view of a staged set (Queries.view)."""

    def __init__(self, parent: Queries, first, count):
        self.ctx = parent.ctx
        self.parent = parent  # (keeps the buffers it points at alive)
        self.seqs = parent.seqs[first:first + count]
        self._h = _P()
        self.ctx._check(load().andi_hip_queries_view(self.ctx._h, parent._h, int(first), int(count), C.byref(self._h)),
                        "queries_view")


def match_positions(esa: Esa, queries: Queries, qidx, first, count, cached=True):
    """get_match(_cached) (src/esa.c:615-656) for consecutive suffixes.
    Returns int32 array (count, 4): l, i, j, SA[i]."""
    if not esa.reference_built:
        esa.build_reference()
    out = np.empty((count, 4), np.int32)
    esa.ctx._check(load().andi_hip_match_positions(esa.ctx._h, esa._h, queries._h, qidx, first, count,
                                                   int(cached), out.ctypes.data), "match_positions")
    return out


def _hook(name):
    fn = getattr(load(), name, None)
    if fn is None:
        raise AndiHipError(name + ": a test hook, not in " + LIB_PATH)
    return fn


def build_indexes(ctx: Context, esas):
    """the scan indexes (probe tables) of several subjects in one pair of launches"""
    n = len(esas)
    hs = (_P * n)(*[e._h for e in esas])
    ctx._check(load().andi_hip_esa_build_index_batch(ctx._h, hs, n), "esa_build_index_batch")


def scan_rows_dev(ctx: Context, esas, selfs, queries: Queries, model, segment, dptr):
    n = len(esas)
    hs = (_P * n)(*[e._h for e in esas])
    sf = (C.c_int64 * n)(*[int(s) for s in selfs])
    ctx._check(load().andi_hip_scan_rows(ctx._h, hs, sf, n, queries._h, model, segment, dptr), "scan_rows")


def scan_rows(ctx: Context, esas, selfs, queries: Queries, model=M_JC, segment=0):
    """dist_anchor (src/process.c:141) for every (subject, query): uint32 array
    (nsub, nq, 17) = 16 counts + seq_len."""
    nsub, nq = len(esas), len(queries)
    out = np.empty((nsub, nq, 17), np.uint32)
    d = ctx.alloc(out.nbytes)
    try:
        scan_rows_dev(ctx, esas, selfs, queries, model, segment, d)
        ctx._check(load().andi_hip_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes), "copy_to_host")
    finally:
        ctx.free(d)
    return out


def device_count():
    return load().andi_hip_device_count()


def pack_symbols(seq: bytes):
    """(4-bit symbols of seq as a numpy uint8 array, whether a byte lies outside the alphabet) -- the host packer of the seam."""
    import numpy as np
    out = np.empty((len(seq) + 1) // 2, np.uint8)
    bad = load().andi_hip_pack_symbols(seq, len(seq), out.ctypes.data_as(C.c_void_p))
    return out, bool(bad)


def trim():
    """Give the device-memory chunks nobody holds a block of back to the driver; returns the bytes released."""
    return int(load().andi_hip_trim())


def reload_knobs():
    """The library reads its ANDI_* environment switches once; read them again (after changing os.environ)."""
    load().andi_hip_reload_knobs()


def last_gather():
    return load().andi_hip_last_gather().decode()


def row_block(total, parts, k):
    """the seam's own tiling of the subject rows over `parts` devices (seam.hip: row_block): [first, last) of part k"""
    f, l = C.c_size_t(0), C.c_size_t(0)
    load().andi_hip_row_block(total, parts, k, C.byref(f), C.byref(l))
    return int(f.value), int(l.value)


def copy_ceiling(ctx, nbytes=1 << 30, reps=5):
    """GB/s (read + written) of the engine's 16-byte streaming copy kernel over nbytes: the measured ceiling beside the
    nominal HBM peak (include/andi_hip.h: andi_hip_copy_ceiling)"""
    g = C.c_double(0.0)
    ctx._check(load().andi_hip_copy_ceiling(ctx._h, nbytes, reps, C.byref(g)), "copy_ceiling")
    return float(g.value)


def bootstrap(ctx: Context, M, replicates, seed=0):
    """calculate_bootstrap (src/process.c:289): (replicates, n, n, 17) uint32."""
    M = np.ascontiguousarray(M, dtype=np.uint32)
    n = M.shape[0]
    assert M.shape == (n, n, 17)
    B = np.empty((replicates, n, n, 17), np.uint32)
    ctx._check(load().andi_hip_bootstrap(ctx._h, M.ctypes.data, n, seed, replicates, B.ctypes.data), "bootstrap")
    return B


def bootstrap_range(ctx: Context, M, first, count, seed=0):
    """Replicates first ... first + count - 1 of bootstrap's stream (andi_hip_bootstrap_range): (count, n, n, 17) uint32,
    bit for bit bootstrap(ctx, M, first + count, seed)[first:]."""
    M = np.ascontiguousarray(M, dtype=np.uint32)
    n = M.shape[0]
    assert M.shape == (n, n, 17)
    B = np.empty((count, n, n, 17), np.uint32)
    ctx._check(load().andi_hip_bootstrap_range(ctx._h, M.ctypes.data, n, seed, first, count, B.ctypes.data),
               "bootstrap_range")
    return B


def estimate_portable(models, model=M_JC):
    """The portable estimator (andi_hip_estimate_portable) of every model of `models` (..., 17) uint32: float64 of
    shape models.shape[:-1].  The function the device computes in bootstrap_nj; no GPU is touched."""
    m = np.ascontiguousarray(models, dtype=np.uint32)
    assert m.ndim >= 1 and m.shape[-1] == 17
    out = np.empty(m.shape[:-1], np.float64)
    if load().andi_hip_estimate_portable(m.ctypes.data, out.size, model, out.ctypes.data):
        raise AndiHipError("andi_hip_estimate_portable: bad arguments")
    return out


def bootstrap_nj(ctx: Context, M, count, model=M_JC, seed=0, first=0, distances=False):
    """Draw, estimate and join on the device (andi_hip_bootstrap_nj): the trees of replicates first ... first + count - 1
    of bootstrap's stream, as nj_batch's (J, bad) -- and, with distances=True, the (count, n, n) float64 matrices the
    joins started from as a third value.  The replicates never exist as models."""
    M = np.ascontiguousarray(M, dtype=np.uint32)
    n = M.shape[0]
    assert M.shape == (n, n, 17)
    J = np.zeros((count, 1 if n == 2 else max(n - 2, 0)), NJ_JOIN)
    bad = np.zeros(count, np.int64)
    D = np.empty((count, n, n), np.float64) if distances else None
    ctx._check(load().andi_hip_bootstrap_nj(ctx._h, M.ctypes.data, n, model, seed, first, count, J.ctypes.data,
                                            bad.ctypes.data, D.ctypes.data if distances else None), "bootstrap_nj")
    return (J, bad, D) if distances else (J, bad)


def nj(ctx: Context, D):
    """Neighbor-joining of the (n, n) distances D on the device (andi_hip_nj; only the upper triangle is read): the n - 2
    records (one for n = 2) as a structured array of dtype NJ_JOIN."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    J = np.zeros(1 if n == 2 else max(n - 2, 0), NJ_JOIN)
    ctx._check(load().andi_hip_nj(ctx._h, D.ctypes.data, n, J.ctypes.data), "nj")
    return J


def nj_batch(ctx: Context, Ds):
    """Neighbor-joining of the (count, n, n) distances Ds in shared launches (andi_hip_nj_batch): (J, bad) -- J[k] the
    records nj(ctx, Ds[k]) gives, bit for bit, as a (count, nrec) array of dtype NJ_JOIN; bad[k] = -1, or i * n + j of
    matrix k's first non-finite entry, and then J[k] is all zero."""
    Ds = np.ascontiguousarray(Ds, dtype=np.float64)
    assert Ds.ndim == 3 and Ds.shape[1] == Ds.shape[2]
    count, n = Ds.shape[0], Ds.shape[1]
    J = np.zeros((count, 1 if n == 2 else max(n - 2, 0)), NJ_JOIN)
    bad = np.zeros(count, np.int64)
    ctx._check(load().andi_hip_nj_batch(ctx._h, Ds.ctypes.data, n, count, J.ctypes.data, bad.ctypes.data), "nj_batch")
    return J, bad


# the tree builders andi_hip_tree takes (ANDI_TREE_*)
TREE_METHODS = {"nj": 0, "bionj": 1}


def _tree_method(method):
    if method not in TREE_METHODS:
        raise ValueError("tree method %r: expected nj or bionj" % (method,))
    return TREE_METHODS[method]


def tree(ctx: Context, D, method="nj"):
    """The tree of the (n, n) distances D by neighbor-joining ("nj") or BIONJ ("bionj") on the device (andi_hip_tree): what
    nj returns, and with "nj" the same bytes."""
    method = _tree_method(method)
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    J = np.zeros(1 if n == 2 else max(n - 2, 0), NJ_JOIN)
    ctx._check(load().andi_hip_tree(ctx._h, D.ctypes.data, n, method, J.ctypes.data), "tree")
    return J


def tree_batch(ctx: Context, Ds, method="nj"):
    """The trees of the (count, n, n) distances Ds in shared launches (andi_hip_tree_batch): what nj_batch returns, J[k] the
    records tree(ctx, Ds[k], method) gives, bit for bit."""
    method = _tree_method(method)
    Ds = np.ascontiguousarray(Ds, dtype=np.float64)
    assert Ds.ndim == 3 and Ds.shape[1] == Ds.shape[2]
    count, n = Ds.shape[0], Ds.shape[1]
    J = np.zeros((count, 1 if n == 2 else max(n - 2, 0)), NJ_JOIN)
    bad = np.zeros(count, np.int64)
    ctx._check(load().andi_hip_tree_batch(ctx._h, Ds.ctypes.data, n, count, method, J.ctypes.data, bad.ctypes.data),
               "tree_batch")
    return J, bad


def bootstrap_tree(ctx: Context, M, count, model=M_JC, method="nj", seed=0, first=0, distances=False):
    """bootstrap_nj with the tree builder chosen (andi_hip_bootstrap_tree): the same replicates and distances, joined by
    `method`; what bootstrap_nj returns."""
    method = _tree_method(method)
    M = np.ascontiguousarray(M, dtype=np.uint32)
    n = M.shape[0]
    assert M.shape == (n, n, 17)
    J = np.zeros((count, 1 if n == 2 else max(n - 2, 0)), NJ_JOIN)
    bad = np.zeros(count, np.int64)
    D = np.empty((count, n, n), np.float64) if distances else None
    ctx._check(load().andi_hip_bootstrap_tree(ctx._h, M.ctypes.data, n, model, method, seed, first, count, J.ctypes.data,
                                              bad.ctypes.data, D.ctypes.data if distances else None), "bootstrap_tree")
    return (J, bad, D) if distances else (J, bad)


def linkage(ctx: Context, D, method="average"):
    """Agglomerative clustering of the (n, n) distances D on the device (andi_hip_linkage; only the upper triangle is
    read, a NaN is a pair without a distance): the n - 1 records as a structured array of dtype LINK."""
    method = _method(method)
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    Z = np.zeros(max(n - 1, 0), LINK)
    ctx._check(load().andi_hip_linkage(ctx._h, D.ctypes.data, n, method, Z.ctypes.data), "linkage")
    return Z


def linkage_batch(ctx: Context, Ds, method="average"):
    """The clustering of the (count, n, n) distances Ds in shared launches (andi_hip_linkage_batch): (Z, bad) -- Z[k] the
    records linkage(ctx, Ds[k], method) gives, bit for bit, as a (count, n - 1) array of dtype LINK; bad[k] = -1, or
    i * n + j of matrix k's first -inf entry, and then Z[k] is all zero."""
    method = _method(method)
    Ds = np.ascontiguousarray(Ds, dtype=np.float64)
    assert Ds.ndim == 3 and Ds.shape[1] == Ds.shape[2]
    count, n = Ds.shape[0], Ds.shape[1]
    Z = np.zeros((count, max(n - 1, 0)), LINK)
    bad = np.zeros(count, np.int64)
    ctx._check(load().andi_hip_linkage_batch(ctx._h, Ds.ctypes.data, n, count, method, Z.ctypes.data,
                                             bad.ctypes.data), "linkage_batch")
    return Z, bad


# andi_hip_fill: a missing pair of andi_hip_complete (its value, the round that filled it -- 0: none did -- and its quartets)
FILL = np.dtype([("i", "<u4"), ("j", "<u4"), ("round", "<u4"), ("pad", "<u4"), ("quartets", "<u8"), ("value", "<f8")])


def complete(ctx: Context, D, max_rounds=0):
    """The missing distances (NaN, +inf, -inf) of the (n, n) matrix D estimated from quartets on the device
    (andi_hip_complete; only the upper triangle is read): (C, fills) -- C the completed matrix, mirrored, a pair that could
    not be derived a NaN; fills one record of dtype FILL per missing pair of D in row-major order, round 0 where it stayed
    missing.  max_rounds = 0: rounds until one fills nothing."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    iu = np.triu_indices(n, 1)
    cap = int((~np.isfinite(D[iu])).sum())
    Cm = np.empty((n, n), np.float64)
    fills = np.zeros(cap, FILL)
    missing, left = C.c_size_t(0), C.c_size_t(0)
    ctx._check(load().andi_hip_complete(ctx._h, D.ctypes.data, n, int(max_rounds), Cm.ctypes.data,
                                        fills.ctypes.data if cap else None, cap, C.byref(missing), C.byref(left)), "complete")
    assert missing.value == cap and left.value == int((fills["round"] == 0).sum())
    return Cm, fills


def complete_batch(ctx: Context, Ds, max_rounds=0):
    """complete for the (count, n, n) matrices Ds in shared launches (andi_hip_complete_batch): (Cs, missing, left) -- Cs[k]
    the matrix complete(ctx, Ds[k]) gives, bit for bit; missing[k] and left[k] its missing pairs before and after."""
    Ds = np.ascontiguousarray(Ds, dtype=np.float64)
    assert Ds.ndim == 3 and Ds.shape[1] == Ds.shape[2]
    count, n = Ds.shape[0], Ds.shape[1]
    Cs = np.empty((count, n, n), np.float64)
    missing, left = np.zeros(count, np.uint64), np.zeros(count, np.uint64)
    ctx._check(load().andi_hip_complete_batch(ctx._h, Ds.ctypes.data, n, count, int(max_rounds), Cs.ctypes.data,
                                              missing.ctypes.data, left.ctypes.data), "complete_batch")
    return Cs, missing, left


# andi_hip_delta: a genome's used quartets and the sum of their floor(delta * 2^24)
DELTA = np.dtype([("sum", "<u8"), ("quartets", "<u8")])


def delta_scores(ctx: Context, D):
    """The tree-likeness scores of the (n, n) matrix D from all its quartets on the device (andi_hip_delta_scores; only the
    upper triangle is read, a pair that is not finite is missing): an (n,) array of dtype DELTA -- per genome the number of
    quartets with six known distances that contain it and the sum of their floor(delta * 2^24), delta = (a - b) / (a - c) of
    the quartet's three sums a >= b >= c.  A genome's mean delta is sum / (quartets * 2^24)."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    out = np.zeros(n, DELTA)
    ctx._check(load().andi_hip_delta_scores(ctx._h, D.ctypes.data, n, out.ctypes.data), "delta_scores")
    return out


def place(ctx: Context, J, D, method="fm", per=False):
    """Distance-based placement (andi_hip_place) of the rows of D (nq, n) -- each a query's distances to the n leaves, a
    NaN where there is none -- on the tree J (n - 2 records of nj or parse_newick): a structured array of dtype PLACEMENT,
    one record per query (edge -1: not placed); with per=True also the (nq, 2n - 3) float64 arrays err, x and p of every
    edge.  method: "fm" (weights 1 / d^2) or "ols"."""
    m = _place_method(method)
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    n = len(J) + 2
    D = np.ascontiguousarray(D, dtype=np.float64)
    assert D.ndim == 2 and D.shape[1] == n
    nq, E = D.shape[0], 2 * n - 3
    out = np.zeros(nq, PLACEMENT)
    rows = [np.zeros((nq, E), np.float64) for _ in range(3)] if per else [None] * 3
    ctx._check(load().andi_hip_place(ctx._h, J.ctypes.data, n, D.ctypes.data, nq, m, out.ctypes.data,
                                     *[r.ctypes.data if per else None for r in rows]), "place")
    return (out, *rows) if per else out


# andi_hip_root_result: the root of a tree (the edge and the distance from its child end), MAD's sum of squared deviations
# there, the used leaf pairs, the least sum among the other edges, and the used pair of the greatest path length
ROOT = np.dtype([("edge", "<i4"), ("pad", "<u4"), ("distal", "<f8"), ("ss", "<f8"), ("pairs", "<u8"), ("ss_second", "<f8"),
                 ("far_b", "<i4"), ("far_c", "<i4")])
ROOT_METHODS = {"mad": 0, "midpoint": 1}


def root(ctx: Context, J, method="mad", per=False):
    """The root of the tree J (n - 2 records of nj, tree or parse_newick) on the device (andi_hip_root): a record of dtype
    ROOT -- the edge, the distance `distal` from its child end, and under "mad" the sum ss of squared deviations there, the
    number of used leaf pairs and the least sum among the other edges (the score is sqrt(ss / pairs), the root ambiguity
    index sqrt(ss / ss_second)); under "midpoint" ss and ss_second are 0.  With per=True (mad only) also the (2n - 3,)
    float64 arrays x and ss of every edge."""
    if str(method).lower() not in ROOT_METHODS:
        raise ValueError("method must be one of %s" % sorted(ROOT_METHODS))
    m = ROOT_METHODS[str(method).lower()]
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    n = len(J) + 2
    out = np.zeros(1, ROOT)
    rows = [np.zeros(2 * n - 3, np.float64) for _ in range(2)] if per else [None] * 2
    ctx._check(load().andi_hip_root(ctx._h, J.ctypes.data, n, m, out.ctypes.data,
                                    *[r.ctypes.data if per else None for r in rows]), "root")
    return (out[0], *rows) if per else out[0]


def newick_rooted(joins, names, edge, distal, labels=None, truncate_names=False):
    """The Newick line of nj's records rooted on `edge`, `distal` from its child end (andi_hip_format_newick_rooted);
    labels: None, or n - 3 strings (or None) that belong to the edges above the pair records' nodes and move with them; ""
    where the library refuses (malformed records, an edge out of range)."""
    J = np.ascontiguousarray(joins, dtype=NJ_JOIN)
    n = len(names)
    cn = _names(names)
    cl, extra = None, 0
    if labels is not None:
        assert len(labels) >= max(n - 3, 0)
        enc = [None if x is None else str(x).encode() for x in labels[:max(n - 3, 0)]]
        cl = (C.c_char_p * max(len(enc), 1))(*enc)
        extra = 2 * sum(len(x) + 1 for x in enc if x is not None)
    cap = 96 + 40 * n + sum(len(x) for x in names) + extra
    for _ in range(2):  # (the call returns the bytes it needs)
        out = C.create_string_buffer(cap)
        need = load().andi_hip_format_newick_rooted(J.ctypes.data, n, cn, int(truncate_names), int(edge), float(distal), cl,
                                                    C.cast(out, _P), cap)
        if need < cap:
            break
        cap = need + 1
    return out.value.decode()


# andi_hip_fit_result: how well a tree explains its matrix -- the residual sums of squares under the refit lengths and
# under the records' own, the total sum of squares, the trees' lengths and negative branches, the worst-fitted pair
FIT = np.dtype([("rss", "<f8"), ("rss_joined", "<f8"), ("tss", "<f8"), ("length", "<f8"), ("length_joined", "<f8"),
                ("worst", "<f8"), ("pairs", "<u8"), ("negative", "<u4"), ("negative_joined", "<u4"), ("worst_b", "<i4"),
                ("worst_c", "<i4")])
FIT_METHODS = ("ols",)


def fit(ctx: Context, J, D, method="ols", per=False):
    """The branch lengths of the tree J (n - 2 records of nj, tree or parse_newick) refit to the (n, n) matrix D by least
    squares on the device (andi_hip_fit): (len, record) -- the (2n - 3,) float64 lengths by edge and a record of dtype
    FIT (R^2 is 1 - rss / tss) --, and with per=True also the (n,) float64 arrays leaf_ss and leaf_ss_joined, every
    genome's share of rss and of rss_joined.  relength puts the lengths into the records."""
    if str(method).lower() not in FIT_METHODS:
        raise ValueError("method must be one of %s" % sorted(FIT_METHODS))
    m = FIT_METHODS.index(str(method).lower())
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    n = len(J) + 2
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.shape != (n, n):
        raise ValueError("D must be (n, n) for the n - 2 records of J")
    length = np.zeros(2 * n - 3, np.float64)
    out = np.zeros(1, FIT)
    rows = [np.zeros(n, np.float64) for _ in range(2)] if per else [None] * 2
    ctx._check(load().andi_hip_fit(ctx._h, J.ctypes.data, n, D.ctypes.data, m, length.ctypes.data, out.ctypes.data,
                                   *[r.ctypes.data if per else None for r in rows]), "fit")
    return (length, out[0], *rows) if per else (length, out[0])


def relength(J, length):
    """The records J with their branch lengths replaced by length[child], the (2n - 3,) lengths by edge
    (andi_hip_relength); raises ValueError where the library refuses (malformed records)."""
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    n = len(J) + 2
    length = np.ascontiguousarray(length, dtype=np.float64)
    if length.shape != (2 * n - 3,):
        raise ValueError("length must hold 2n - 3 values")
    out = np.zeros(len(J), NJ_JOIN)
    if load().andi_hip_relength(J.ctypes.data, n, length.ctypes.data, out.ctypes.data):
        raise ValueError("andi_hip_relength: the records are not those of andi_hip_nj")
    return out


# andi_hip_refine_result and andi_hip_refine_move: the sums of the balanced lengths before and after the search, the moves
# made and whether it converged; a move's gain and the least leaves of the two subtrees it swapped
REFINE = np.dtype([("length_before", "<f8"), ("length_after", "<f8"), ("moves", "<u8"), ("converged", "<i4"), ("pad", "<i4")])
REFINE_MOVE = np.dtype([("gain", "<f8"), ("first", "<i4"), ("second", "<i4")])
REFINE_METHODS = ("bnni",)


def refine(ctx: Context, J, D, method="bnni", tol=0.0, max_moves=None, log=False):
    """The tree J (n - 2 records of nj, tree or parse_newick) refined against the (n, n) matrix D by balanced
    nearest-neighbor interchanges on the device (andi_hip_refine): (records, result) -- the refined tree's records with
    its balanced lengths and a record of dtype REFINE --, and with log=True also the moves made, an array of dtype
    REFINE_MOVE.  A move is made only if it shortens the tree by more than tol; max_moves=None allows 10 n."""
    if str(method).lower() not in REFINE_METHODS:
        raise ValueError("method must be one of %s" % sorted(REFINE_METHODS))
    m = REFINE_METHODS.index(str(method).lower())
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    n = len(J) + 2
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.shape != (n, n):
        raise ValueError("D must be (n, n) for the n - 2 records of J")
    cap = 10 * n if max_moves is None else int(max_moves)
    if cap < 0:
        raise ValueError("max_moves must not be negative")
    out = np.zeros(len(J), NJ_JOIN)
    res = np.zeros(1, REFINE)
    moves = np.zeros(max(cap, 1), REFINE_MOVE) if log else None
    ctx._check(load().andi_hip_refine(ctx._h, J.ctypes.data, n, D.ctypes.data, m, float(tol), cap, out.ctypes.data,
                                      res.ctypes.data, moves.ctypes.data if log else None), "refine")
    return (out, res[0], moves[:int(res[0]["moves"])].copy()) if log else (out, res[0])


# andi_hip_spr_move: a move's gain, the least leaves of the pruned side and of the side beyond the target edge, the hops
SPR_MOVE = np.dtype([("gain", "<f8"), ("first", "<i4"), ("second", "<i4"), ("hops", "<i4"), ("pad", "<i4")])


def refine_spr(ctx: Context, J, D, tol=0.0, max_moves=None, log=False):
    """refine() with balanced subtree pruning and regrafting as the move (andi_hip_refine_spr): a round re-hangs one
    subtree on any other branch.  The same arguments and results; the log's entries are of dtype SPR_MOVE."""
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    n = len(J) + 2
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.shape != (n, n):
        raise ValueError("D must be (n, n) for the n - 2 records of J")
    cap = 10 * n if max_moves is None else int(max_moves)
    if cap < 0:
        raise ValueError("max_moves must not be negative")
    out = np.zeros(len(J), NJ_JOIN)
    res = np.zeros(1, REFINE)
    moves = np.zeros(max(cap, 1), SPR_MOVE) if log else None
    ctx._check(load().andi_hip_refine_spr(ctx._h, J.ctypes.data, n, D.ctypes.data, float(tol), cap, out.ctypes.data,
                                          res.ctypes.data, moves.ctypes.data if log else None), "refine_spr")
    return (out, res[0], moves[:int(res[0]["moves"])].copy()) if log else (out, res[0])


def nj_support(ctx: Context, J, reps, skip=None):
    """Bootstrap support (andi_hip_nj_support): for every pair record of the tree J (n - 2 records) the number of the
    replicate trees reps (count, n - 2), but those with skip[k] set, that hold the same bipartition of the leaves:
    uint32[n - 3]."""
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    reps = np.ascontiguousarray(reps, dtype=NJ_JOIN)
    n = len(J) + 2
    assert reps.ndim == 2 and reps.shape[1] == len(J)
    if skip is not None:
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        assert skip.shape == (reps.shape[0],)
    support = np.zeros(max(n - 3, 0), np.uint32)
    ctx._check(load().andi_hip_nj_support(ctx._h, J.ctypes.data, reps.ctypes.data, n, reps.shape[0],
                                          skip.ctypes.data if skip is not None else None, support.ctypes.data),
               "nj_support")
    return support


def nj_transfer(ctx: Context, J, reps, skip=None, per=False):
    """Transfer bootstrap support (andi_hip_nj_transfer) of the tree J (n - 2 records) among the replicate trees reps
    (count, n - 2), but those with skip[k] set: (depth, transfer) -- uint32[n - 3], the size of the smaller side of every
    pair record's bipartition, and uint64[n - 3], its transfer index summed over the used replicates; with per=True also
    the (count, n - 3) uint32 transfer indices themselves (0xFFFFFFFF in a skipped replicate's row)."""
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    reps = np.ascontiguousarray(reps, dtype=NJ_JOIN)
    n = len(J) + 2
    assert reps.ndim == 2 and reps.shape[1] == len(J)
    count = reps.shape[0]
    skip = _skip(skip, count)
    depth = np.zeros(max(n - 3, 0), np.uint32)
    transfer = np.zeros(max(n - 3, 0), np.uint64)
    each = np.zeros((count, max(n - 3, 0)), np.uint32) if per else None
    ctx._check(load().andi_hip_nj_transfer(ctx._h, J.ctypes.data, reps.ctypes.data, n, count,
                                           skip.ctypes.data if skip is not None else None, depth.ctypes.data,
                                           transfer.ctypes.data, each.ctypes.data if per else None), "nj_transfer")
    return (depth, transfer, each) if per else (depth, transfer)


def nj_transfer_taxa(ctx: Context, J, reps, skip=None, cutoff=0.3, detail=False):
    """The rogue genomes of a bootstrap (andi_hip_nj_transfer_taxa): (moved, pairs) -- uint64[n], for every leaf the number
    of counted pairs (replicate, branch of J) in which it is one of the leaves that have to move, and the number of counted
    pairs; a pair counts iff its transfer distance is at most floor(cutoff * (depth - 1)).  With detail=True also match
    and dist, (count, n - 3) uint32: the replicate's nearest pair record (the least in a tie) and its uncapped distance
    (0xFFFFFFFF in a skipped replicate's row)."""
    J = np.ascontiguousarray(J, dtype=NJ_JOIN)
    reps = np.ascontiguousarray(reps, dtype=NJ_JOIN)
    n = len(J) + 2
    assert reps.ndim == 2 and reps.shape[1] == len(J)
    count = reps.shape[0]
    skip = _skip(skip, count)
    moved = np.zeros(n, np.uint64)
    pairs = C.c_uint64(0)
    match = np.zeros((count, max(n - 3, 0)), np.uint32) if detail else None
    dist = np.zeros((count, max(n - 3, 0)), np.uint32) if detail else None
    ctx._check(load().andi_hip_nj_transfer_taxa(ctx._h, J.ctypes.data, reps.ctypes.data, n, count,
                                                skip.ctypes.data if skip is not None else None, float(cutoff),
                                                moved.ctypes.data, C.addressof(pairs), match.ctypes.data if detail else None,
                                                dist.ctypes.data if detail else None), "nj_transfer_taxa")
    return (moved, int(pairs.value), match, dist) if detail else (moved, int(pairs.value))


def nj_splits(ctx: Context, reps, skip=None):
    """Every distinct bipartition among the replicate trees reps (count, n - 2), but those with skip[k] set
    (andi_hip_nj_splits): (ids, freq, sets) -- ids (count, n - 3) uint32, the split of every pair record, numbered by first
    appearance (0xFFFFFFFF in a skipped replicate); freq[id] the replicates that have split id; sets (nsplits, W) uint64,
    its leaf set on the side without leaf 0."""
    reps = np.ascontiguousarray(reps, dtype=NJ_JOIN)
    assert reps.ndim == 2
    count, n = reps.shape[0], reps.shape[1] + 2
    skip = _skip(skip, count)
    ids = np.zeros((count, max(n - 3, 0)), np.uint32)
    nsplits, pf, ps = C.c_size_t(0), _P(), _P()
    ctx._check(load().andi_hip_nj_splits(ctx._h, reps.ctypes.data, n, count, skip.ctypes.data if skip is not None else None,
                                         ids.ctypes.data, C.byref(nsplits), C.byref(pf), C.byref(ps)), "nj_splits")
    W, T = (n + 63) // 64, nsplits.value
    try:
        freq = np.ctypeslib.as_array(C.cast(pf, C.POINTER(C.c_uint32)), (T,)).copy() if T else np.zeros(0, np.uint32)
        sets = np.ctypeslib.as_array(C.cast(ps, C.POINTER(C.c_uint64)), (T, W)).copy() if T else np.zeros((0, W), np.uint64)
    finally:
        load().andi_hip_free(pf)
        load().andi_hip_free(ps)
    return ids, freq, sets


def _opts(p_value, model, device, host_threads, segment, num_gpus, devices, low_memory, sa_on_host, progress=None):
    """(Opts, what must stay alive while it is used)"""
    o = Opts()
    load().andi_hip_default_opts(C.byref(o))
    o.p_value, o.model, o.device, o.host_threads, o.segment = p_value, model, device, host_threads, segment
    o.low_memory = int(low_memory)
    o.sa_on_host = int(sa_on_host)
    o.num_gpus = num_gpus
    if devices is not None:
        dl = (C.c_int * len(devices))(*devices)
        o.devices, o.num_gpus = dl, len(devices)
    keep = [dl] if devices is not None else []
    if progress is not None:
        cb = PROGRESS_FN(lambda done, total, ud: progress(done, total))
        o.progress = cb
        keep.append(cb)
    return o, keep


def dist_matrix(seqs, p_value=0.025, model=M_JC, device=0, host_threads=0, segment=0, num_gpus=1, devices=None,
                low_memory=False, sa_on_host=False):
    """distMatrix (src/dist_hack.h:34): n*n*17 uint32, row = subject.  num_gpus / devices: the rows are
    tiled over several devices (or several contexts on one) behind the same call."""
    L = load()
    seqs = [bytes(s) for s in seqs]
    n = len(seqs)
    arr = _seq_array(seqs)
    o, _keep = _opts(p_value, model, device, host_threads, segment, num_gpus, devices, low_memory, sa_on_host)
    M = np.zeros((n, n, 17), np.uint32)
    err = C.create_string_buffer(512)
    if L.andi_hip_dist_matrix(M.ctypes.data, arr, n, C.byref(o), err, len(err)):
        raise AndiHipError(err.value.decode())
    return M


def dist_rect(refs, queries, p_value=0.025, model=M_JC, device=0, host_threads=0, segment=0, num_gpus=1, devices=None,
              low_memory=False, sa_on_host=False, progress=None):
    """The query-versus-reference mode (andi_hip_dist_rect): (MRQ, MQR), uint32 arrays (nr, nq, 17) and (nq, nr, 17) --
    the cross blocks M[:nr, nr:] and M[nr:, :nr] of dist_matrix(refs + queries), bit for bit, computed alone.
    progress(done, total): called from the devices' driver threads, total = 2 * nr * nq."""
    L = load()
    refs = [bytes(s) for s in refs]
    queries = [bytes(s) for s in queries]
    nr, nq = len(refs), len(queries)
    ra, qa = _seq_array(refs), _seq_array(queries)
    o, _keep = _opts(p_value, model, device, host_threads, segment, num_gpus, devices, low_memory, sa_on_host, progress)
    MRQ = np.zeros((nr, nq, 17), np.uint32)
    MQR = np.zeros((nq, nr, 17), np.uint32)
    err = C.create_string_buffer(512)
    if L.andi_hip_dist_rect(MRQ.ctypes.data, MQR.ctypes.data, ra, nr, qa, nq, C.byref(o), err, len(err)):
        raise AndiHipError(err.value.decode())
    return MRQ, MQR


# ---------------------------------------------------------------- the k-mer sketch screen
class Sketches:
    """The sketches of a set of sequences, resident on the context's device (andi_hip_sketch): len(), .sizes (uint32),
    .hashes(i) (uint64, ascending), .timings() (ms: pack, upload, hash, sort), close()."""

    def __init__(self, ctx: Context, seqs, k=21, scale=1000):
        seqs = [bytes(s) for s in seqs]
        arr = _seq_array(seqs) if seqs else None
        self._ctx, self._h = ctx, _P()
        self.k, self.scale = int(k), int(scale)
        if not 0 <= int(scale) < 1 << 64:
            raise AndiHipError("sketch: scale %r does not fit 64 bits" % (scale,))
        ctx._check(load().andi_hip_sketch(ctx._h, arr, len(seqs), int(k), int(scale), C.byref(self._h)), "sketch")
        n = load().andi_hip_sketch_count(self._h)
        self.sizes = np.zeros(n, np.uint32)
        ctx._check(load().andi_hip_sketch_sizes(ctx._h, self._h, self.sizes.ctypes.data), "sketch_sizes")

    def __len__(self):
        return len(self.sizes)

    def hashes(self, i):
        out = np.zeros(int(self.sizes[i]), np.uint64)
        self._ctx._check(load().andi_hip_sketch_download(self._ctx._h, self._h, int(i), out.ctypes.data), "sketch_download")
        return out

    def timings(self):
        ms = np.zeros(4, np.float64)
        load().andi_hip_sketch_timings(self._h, ms.ctypes.data)
        return dict(zip(("pack_ms", "upload_ms", "hash_ms", "sort_ms"), ms.tolist()))

    def close(self):
        if self._h and self._ctx._h:
            load().andi_hip_sketch_free(self._ctx._h, self._h)
        self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sketch(ctx: Context, seqs, k=21, scale=1000):
    """andi_hip_sketch: the sketches of seqs (bytes over A C G T !) at k-mer length k and the given scale (the defaults are
    sourmash's), as a Sketches object."""
    return Sketches(ctx, seqs, k, scale)


def sketch_shared(ctx: Context, A: Sketches, B: Sketches):
    """andi_hip_sketch_shared: the uint32 array (len(A), len(B)) of the numbers of hashes sketch i of A and sketch j of B share."""
    out = np.zeros((len(A), len(B)), np.uint32)
    ctx._check(load().andi_hip_sketch_shared(ctx._h, A._h, B._h, out.ctypes.data), "sketch_shared")
    return out


def screen_select(shared, keep, min_shared=1):
    """andi_hip_screen_select on the (nq, nr) counts: (kept, taken) -- kept[r] (bool) iff some query took reference r among its
    best `keep` with at least max(1, min_shared) shared hashes, taken[q] (uint32) how many query q took.  No GPU."""
    shared = np.ascontiguousarray(shared, dtype=np.uint32)
    if shared.ndim != 2:
        raise ValueError("screen_select: shared must be (nq, nr)")
    nq, nr = shared.shape
    kept, taken = np.zeros(nr, np.uint8), np.zeros(nq, np.uint32)
    if load().andi_hip_screen_select(shared.ctypes.data, nq, nr, int(keep), int(min_shared), kept.ctypes.data, taken.ctypes.data):
        raise AndiHipError("screen_select: bad arguments (nq and nr must be at least 1)")
    return kept.astype(bool), taken


def screen(refs, queries, k=21, scale=1000, device=0):
    """andi_hip_screen, the one call: (shared (nq, nr) uint32, ref_sizes, query_sizes)."""
    refs = [bytes(s) for s in refs]
    queries = [bytes(s) for s in queries]
    nr, nq = len(refs), len(queries)
    shared = np.zeros((nq, nr), np.uint32)
    rs, qs = np.zeros(nr, np.uint32), np.zeros(nq, np.uint32)
    err = C.create_string_buffer(512)
    if load().andi_hip_screen(_seq_array(refs) if refs else None, nr, _seq_array(queries) if queries else None, nq, int(k), int(scale),
                              int(device), shared.ctypes.data, rs.ctypes.data, qs.ctypes.data, err, len(err)):
        raise AndiHipError(err.value.decode(errors="replace"))
    return shared, rs, qs
