"""ctypes binding of libbls12_381_mi355x.so (the C ABI in include/bls12_381_mi355x.h).

Thin: config structs, error mapping, and numpy/torch conveniences for tests and bench.
There is no CPU fallback -- if the HIP library is missing or fails to load this module raises.
Device buffers are torch tensors (torch is plumbing here: allocation + streams)."""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MBLS_LIB: an alternative in-tree build of the same library (A/B tuning runs only)
LIB_PATH = os.environ.get("MBLS_LIB") or os.path.join(HERE, "lib", "libbls12_381_mi355x.so")

ERRORS = ["SUCCESS", "INVALID_DEVICE", "OUT_OF_MEMORY", "INVALID_POINTER", "ALLOCATION_FAILED",
          "DEALLOCATION_FAILED", "COPY_FAILED", "SYNCHRONIZATION_FAILED", "STREAM_CREATION_FAILED",
          "STREAM_DESTRUCTION_FAILED", "API_NOT_IMPLEMENTED", "INVALID_ARGUMENT", "BACKEND_LOAD_FAILED",
          "LICENSE_CHECK_ERROR", "UNKNOWN_ERROR"]
SUCCESS, INVALID_POINTER, API_NOT_IMPLEMENTED, INVALID_ARGUMENT = 0, 3, 10, 11


class IcicleError(RuntimeError):
    def __init__(self, code, what):
        name = ERRORS[code] if 0 <= code < len(ERRORS) else str(code)
        super().__init__(f"{what} failed: {name} ({code})")
        self.code = code


class MSMConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("precompute_factor", ctypes.c_int), ("c", ctypes.c_int),
                ("bitsize", ctypes.c_int), ("batch_size", ctypes.c_int),
                ("are_points_shared_in_batch", ctypes.c_bool), ("are_scalars_on_device", ctypes.c_bool),
                ("are_scalars_montgomery_form", ctypes.c_bool), ("are_points_on_device", ctypes.c_bool),
                ("are_points_montgomery_form", ctypes.c_bool), ("are_results_on_device", ctypes.c_bool),
                ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


class FrC(ctypes.Structure):
    _fields_ = [("limbs", ctypes.c_uint64 * 4)]


class NTTConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("coset_gen", FrC), ("batch_size", ctypes.c_int),
                ("columns_batch", ctypes.c_bool), ("ordering", ctypes.c_int),
                ("are_inputs_on_device", ctypes.c_bool), ("are_outputs_on_device", ctypes.c_bool),
                ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


class NTTInitDomainConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("is_async", ctypes.c_bool), ("ext", ctypes.c_void_p)]


class VecOpsConfig(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_void_p), ("is_a_on_device", ctypes.c_bool), ("is_b_on_device", ctypes.c_bool),
                ("is_result_on_device", ctypes.c_bool), ("is_async", ctypes.c_bool), ("batch_size", ctypes.c_int),
                ("columns_batch", ctypes.c_bool), ("ext", ctypes.c_void_p)]


# every symbol include/bls12_381_mi355x.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "mbls_default_msm_config", "mbls_default_ntt_config", "mbls_default_vec_ops_config",
    "bls12_381_g1_msm_cuda", "bls12_381_g2_msm_cuda", "bls12_381_icicle_g1_msm", "bls12_381_icicle_g2_msm",
    "bls12_381_icicle_g1_msm_precompute_bases", "bls12_381_icicle_g2_msm_precompute_bases",
    "bls12_381_ntt_init_domain_cuda", "bls12_381_ntt_release_domain_cuda", "bls12_381_ntt_cuda",
    "bls12_381_coset_ntt_cuda", "bls12_381_field_ntt_cuda", "bls12_381_field_ntt_init_domain_cuda",
    "bls12_381_field_ntt_release_domain_cuda", "bls12_381_ntt_get_rou_from_domain",
    "bls12_381_vector_add", "bls12_381_vector_sub", "bls12_381_vector_mul", "bls12_381_scalar_mul_vec",
    "bls12_381_scalar_add_vec", "vec_add_cuda", "vec_sub_cuda", "vec_mul_cuda", "scalar_mul_vec_cuda",
    "scalar_add_vec_cuda", "vec_sum_cuda", "bls12_381_batch_inv_cuda",
    "mbls_version", "mbls_error_string", "mbls_gen_scalars", "mbls_gen_g1_bases", "mbls_gen_g2_bases",
    "mbls_gen_scalars_range", "mbls_gen_g1_bases_range", "mbls_gen_g2_bases_range",
    "mbls_g1_msm_jacobian", "mbls_g2_msm_jacobian",
    "mbls_g1_sum_jacobian", "mbls_g2_sum_jacobian", "mbls_g1_jacobian_to_icicle", "mbls_g2_jacobian_to_icicle",
    "mbls_profile_enable", "mbls_profile_reset", "mbls_profile_read",
    "mbls_release_stream", "mbls_release_scratch", "mbls_scratch_stats",
    "mbls_g1_msm_multi_device", "mbls_g2_msm_multi_device", "bls12_381_vector_sum",
    "bls12_381_g1_affine_to_projective", "bls12_381_g1_projective_to_affine", "bls12_381_g2_projective_to_affine",
    "mbls_msm_plan", "mbls_msm_reduce_plan", "mbls_msm_front_probe", "mbls_msm_accumulate_event", "mbls_msm_accumulate_event_drop", "mbls_msm_precompute_strict",
    "bls12_381_g1_scalar_mul", "bls12_381_g1_scalar_mul_glv", "bls12_381_g2_scalar_mul",
    "mbls_g1_scalar_mul", "mbls_g2_scalar_mul", "mbls_g1_ecntt",
    "mbls_g1_check_points", "mbls_g2_check_points",
    "mbls_g1_decompress", "mbls_g2_decompress", "mbls_g1_compress", "mbls_g2_compress",
    "mbls_fr_prefix_product", "mbls_fr_poly_divide_linear", "mbls_fr_scan_geometry",
    "mbls_fr_eval_program", "mbls_fr_expr_check", "mbls_fr_eval_graph", "mbls_fr_graph_check",
    "mbls_fr_sort", "mbls_fr_lookup_permute", "mbls_fr_sort_plan",
    "mbls_fr_coeff_to_extended", "mbls_fr_extended_to_coeff", "mbls_fr_domain_plan",
    "mbls_fr_lookup_multiplicities", "mbls_fr_prefix_sum", "mbls_fr_logup_sum",
    "mbls_fr_inner_products", "mbls_fr_multi_eval", "mbls_fr_powers", "mbls_fr_inner_plan",
    "mbls_fixed_base_plan", "mbls_fixed_base_recode", "mbls_g1_fixed_base_table", "mbls_g2_fixed_base_table",
    "mbls_g1_fixed_base_mul", "mbls_g2_fixed_base_mul", "mbls_g1_srs_from_secret",
]

_LIB = None


def lib():
    """Load the HIP library (raises if it is missing: there is no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"HIP library not built: {LIB_PATH} (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    P, E = ctypes.c_void_p, ctypes.c_int
    sz, i32, u64, b = ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64, ctypes.c_bool
    sig = {
        "bls12_381_g1_msm_cuda": [P, P, i32, P, P], "bls12_381_g2_msm_cuda": [P, P, i32, P, P],
        "bls12_381_icicle_g1_msm": [P, P, i32, P, P], "bls12_381_icicle_g2_msm": [P, P, i32, P, P],
        "bls12_381_icicle_g1_msm_precompute_bases": [P, i32, P, P],
        "bls12_381_icicle_g2_msm_precompute_bases": [P, i32, P, P],
        "bls12_381_ntt_init_domain_cuda": [P, P], "bls12_381_ntt_release_domain_cuda": [],
        "bls12_381_ntt_cuda": [P, i32, i32, P, P], "bls12_381_coset_ntt_cuda": [P, i32, i32, P, P, P],
        "bls12_381_field_ntt_cuda": [P, i32, i32, P, P], "bls12_381_field_ntt_init_domain_cuda": [P, P],
        "bls12_381_field_ntt_release_domain_cuda": [], "bls12_381_ntt_get_rou_from_domain": [u64, P],
        "bls12_381_vector_add": [P, P, sz, P, P], "bls12_381_vector_sub": [P, P, sz, P, P],
        "bls12_381_vector_mul": [P, P, sz, P, P], "bls12_381_scalar_mul_vec": [P, P, sz, P, P],
        "bls12_381_scalar_add_vec": [P, P, sz, P, P],
        "vec_add_cuda": [P, P, P, i32, P], "vec_sub_cuda": [P, P, P, i32, P], "vec_mul_cuda": [P, P, P, i32, P],
        "scalar_mul_vec_cuda": [P, P, P, i32, P], "scalar_add_vec_cuda": [P, P, P, i32, P],
        "vec_sum_cuda": [P, P, i32, P], "bls12_381_batch_inv_cuda": [P, P, i32, P],
        "mbls_gen_scalars": [P, u64, sz, b, P], "mbls_gen_g1_bases": [P, u64, sz, P],
        "mbls_gen_g2_bases": [P, u64, sz, P], "mbls_g1_sum_jacobian": [P, i32, P, P],
        "mbls_gen_scalars_range": [P, u64, sz, sz, b, P], "mbls_gen_g1_bases_range": [P, u64, sz, sz, P],
        "mbls_gen_g2_bases_range": [P, u64, sz, sz, P],
        "mbls_g1_msm_jacobian": [P, P, i32, P, P], "mbls_g2_msm_jacobian": [P, P, i32, P, P],
        "mbls_g2_sum_jacobian": [P, i32, P, P], "mbls_g1_jacobian_to_icicle": [P, i32, P],
        "mbls_g2_jacobian_to_icicle": [P, i32, P],
        "mbls_release_stream": [P], "mbls_release_scratch": [],
        "mbls_g1_msm_multi_device": [P, P, P, i32, i32, P, P], "mbls_g2_msm_multi_device": [P, P, P, i32, i32, P, P],
        "bls12_381_vector_sum": [P, sz, P, P],
        "bls12_381_g1_affine_to_projective": [P, i32, P, P], "bls12_381_g1_projective_to_affine": [P, i32, P, P],
        "bls12_381_g2_projective_to_affine": [P, i32, P, P],
        "mbls_msm_plan": [i32, i32, P, P], "mbls_msm_reduce_plan": [i32, i32, P, P, i32, P],
        "mbls_msm_front_probe": [i32, P, P, i32, P, P, P],
        "mbls_msm_accumulate_event": [P, P], "mbls_msm_accumulate_event_drop": [P],
        "mbls_msm_precompute_strict": [i32],
        "bls12_381_g1_scalar_mul": [P, P, i32, P, P], "bls12_381_g1_scalar_mul_glv": [P, P, i32, P, P],
        "bls12_381_g2_scalar_mul": [P, P, i32, P, P],
        "mbls_g1_scalar_mul": [P, P, i32, b, P, P], "mbls_g2_scalar_mul": [P, P, i32, b, P, P],
        "mbls_g1_ecntt": [P, i32, i32, P, P],
        "mbls_g1_check_points": [P, i32, b, P, P, P], "mbls_g2_check_points": [P, i32, b, P, P, P],
        "mbls_g1_decompress": [P, i32, b, P, P, P, P], "mbls_g2_decompress": [P, i32, b, P, P, P, P],
        "mbls_g1_compress": [P, i32, b, P, P], "mbls_g2_compress": [P, i32, b, P, P],
        "mbls_fr_prefix_product": [P, P, sz, P, b, P, P, P], "mbls_fr_poly_divide_linear": [P, sz, P, P, P, P],
        "mbls_fr_scan_geometry": [sz, P],
        "mbls_fr_eval_program": [P, i32, sz, sz, P, i32, P, i32, i32, P, P],
        "mbls_fr_expr_check": [P, i32, i32, i32, i32, P],
        "mbls_fr_eval_graph": [P, i32, sz, sz, P, i32, P, i32, i32, P, P],
        "mbls_fr_graph_check": [P, i32, i32, i32, i32, P],
        "mbls_fr_sort": [P, sz, b, P, P, P], "mbls_fr_lookup_permute": [P, P, sz, b, P, P, P, P],
        "mbls_fr_sort_plan": [sz, i32, P],
        "mbls_fr_coeff_to_extended": [P, i32, i32, P, P, P],
        "mbls_fr_extended_to_coeff": [P, i32, i32, P, P, i32, P, P], "mbls_fr_domain_plan": [i32, i32, P],
        "mbls_fr_lookup_multiplicities": [P, i32, P, sz, b, b, P, P, P],
        "mbls_fr_prefix_sum": [P, sz, P, b, P, P, P], "mbls_fr_logup_sum": [P, i32, P, P, sz, P, P, P, P, P],
        "mbls_fr_inner_products": [P, i32, P, i32, sz, P, P], "mbls_fr_multi_eval": [P, i32, sz, P, i32, P, P],
        "mbls_fr_powers": [P, P, sz, P, P], "mbls_fr_inner_plan": [sz, i32, i32, P],
        "mbls_fixed_base_plan": [i32, P], "mbls_fixed_base_recode": [P, P],
        "mbls_g1_fixed_base_table": [P, P, P], "mbls_g2_fixed_base_table": [P, P, P],
        "mbls_g1_fixed_base_mul": [P, P, i32, b, P, P], "mbls_g2_fixed_base_mul": [P, P, i32, b, P, P],
        "mbls_g1_srs_from_secret": [P, P, i32, i32, P, P],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = E
    L.mbls_version.restype = ctypes.c_char_p
    L.mbls_error_string.restype = ctypes.c_char_p
    L.mbls_error_string.argtypes = [E]
    L.mbls_default_msm_config.restype = MSMConfig
    L.mbls_default_ntt_config.restype = NTTConfig
    L.mbls_default_vec_ops_config.restype = VecOpsConfig
    L.mbls_profile_enable.argtypes = [ctypes.c_int]
    L.mbls_profile_enable.restype = None
    L.mbls_profile_reset.argtypes = []
    L.mbls_profile_reset.restype = None
    L.mbls_profile_read.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_long), ctypes.c_int]
    L.mbls_profile_read.restype = ctypes.c_int
    L.mbls_scratch_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64)] * 3 + [ctypes.POINTER(ctypes.c_int)]
    L.mbls_scratch_stats.restype = None
    _LIB = L
    return L


def profile(enable=True):
    lib().mbls_profile_enable(1 if enable else 0)
    lib().mbls_profile_reset()


def profile_read():
    """{stage: (total_ms, launches)} since the last profile()/reset"""
    n = 64
    names = (ctypes.c_char_p * n)()
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_long * n)()
    k = lib().mbls_profile_read(names, ms, cnt, n)
    return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(k, n))}


def check(code, what):
    if code != SUCCESS:
        raise IcicleError(code, what)


def _p(x):
    """pointer of a numpy array or torch tensor"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return ctypes.c_void_p(x.ctypes.data)
    return ctypes.c_void_p(x.data_ptr())


def _is_dev(x):
    """device operand: a torch tensor on the GPU (numpy arrays and CPU / pinned torch tensors
    are host memory)"""
    return x is not None and not isinstance(x, np.ndarray) and bool(getattr(x, "is_cuda", True))


def _stream_handle(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


# ----------------------------------------------------------------------------- configs
def msm_config(**kw):
    c = lib().mbls_default_msm_config()
    for k, v in kw.items():
        if k == "stream":
            c.stream = _stream_handle(v)
        else:
            setattr(c, k, v)
    return c


PLAN_FIELDS = ("c", "W", "Wg", "F", "sF", "split", "prepared", "bstride", "buckets", "levels")


def msm_plan(group, n, **cfg):
    """the MSM schedule the library picks (mbls_msm_plan; host only): dict of PLAN_FIELDS"""
    out = (ctypes.c_int32 * len(PLAN_FIELDS))()
    c = msm_config(**cfg)
    check(lib().mbls_msm_plan(1 if group == "g1" else 2, n, ctypes.byref(c), out), "msm_plan")
    return dict(zip(PLAN_FIELDS, list(out)))


REDUCE_KERNELS = ("chain", "tree4", "r28x", "tree8", "r28px")  # the library's RedKernel ids
REDUCE_MODES = ("lane", "row", "wave")
REDUCE_LEVEL_FIELDS = ("kernel", "launch", "mode", "seg_log", "m_in", "raw_in", "raw_out")


def msm_reduce_plan(group, n, **cfg):
    """the bucket reduction's kernel schedule of msm_plan(group, n, **cfg) (mbls_msm_reduce_plan;
    host only): dict(bucket_raw, level_bytes, levels = [dict of REDUCE_LEVEL_FIELDS]), kernel and
    mode by name"""
    out = (ctypes.c_int32 * 128)()
    cnt = ctypes.c_int32(0)
    c = msm_config(**cfg)
    check(lib().mbls_msm_reduce_plan(1 if group == "g1" else 2, n, ctypes.byref(c), out, len(out), ctypes.byref(cnt)),
          "msm_reduce_plan")
    levels = []
    for k in range(2, cnt.value, len(REDUCE_LEVEL_FIELDS)):
        lv = dict(zip(REDUCE_LEVEL_FIELDS, out[k:k + len(REDUCE_LEVEL_FIELDS)]))
        lv["kernel"], lv["mode"] = REDUCE_KERNELS[lv["kernel"]], REDUCE_MODES[lv["mode"]]
        levels.append(lv)
    return dict(bucket_raw=out[0], level_bytes=out[1], levels=levels)


FRONT_PLAN_FIELDS = ("c", "W", "Wg", "F", "sF", "split", "prepared", "bstride", "B", "TB", "chunk", "pts",
                     "contributions", "partition_sort", "fused_chunk_counts")
FRONT_TABLES = ("sorted", "offsets", "nchunks", "chunk_off", "owner", "first", "perm", "binbase", "H_bucket",
                "H_first", "H_nslices", "H_done", "H_owner", "H_gdone")
FRONT_FILL = 0xA5A5A5A5  # a word of a scratch block the front did not write


def msm_front_plan(group, n, **cfg):
    """the plan msm_front_tables(group, <n scalars>, **cfg) runs and its tables' capacities in words
    (mbls_msm_front_probe without tables; host only): dict(plan, words)"""
    c = msm_config(**cfg)
    info = (ctypes.c_int64 * (len(FRONT_PLAN_FIELDS) + len(FRONT_TABLES)))()
    check(lib().mbls_msm_front_probe(1 if group == "g1" else 2, None, None, n, ctypes.byref(c), info, None),
          "msm_front_probe")
    k = len(FRONT_PLAN_FIELDS)
    return dict(plan=dict(zip(FRONT_PLAN_FIELDS, list(info)[:k])), words=dict(zip(FRONT_TABLES, list(info)[k:])))


def msm_front_tables(group, scalars, bases=None, *, n=None, c=0, bitsize=0, precompute_factor=1, scalars_mont=False,
                     points_mont=True, stream=None):
    """The front's tables of the MSM msm(group, scalars, bases, ...) would run (mbls_msm_front_probe):
    dict(plan = dict of FRONT_PLAN_FIELDS as the call used them, tables = dict of FRONT_TABLES, each a
    uint32 numpy array of its scratch block's full capacity, words the front left alone holding
    FRONT_FILL).  scalars (n, 4) uint64, numpy (host) or torch (device); bases may be None where the
    plan builds no per-call image table."""
    if n is None:
        n = scalars.shape[0]
    cfg = msm_config(c=c, bitsize=bitsize, precompute_factor=precompute_factor,
                     are_scalars_on_device=_is_dev(scalars), are_scalars_montgomery_form=scalars_mont,
                     are_points_on_device=_is_dev(bases), are_points_montgomery_form=points_mont, stream=stream)
    g = 1 if group == "g1" else 2
    info = (ctypes.c_int64 * (len(FRONT_PLAN_FIELDS) + len(FRONT_TABLES)))()
    check(lib().mbls_msm_front_probe(g, None, None, n, ctypes.byref(cfg), info, None), "msm_front_probe")
    words = list(info)[len(FRONT_PLAN_FIELDS):]
    tabs = [np.zeros(w, dtype=np.uint32) for w in words]
    ptrs = (ctypes.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
    check(lib().mbls_msm_front_probe(g, _p(scalars), _p(bases), n, ctypes.byref(cfg), info, ptrs), "msm_front_probe")
    assert list(info)[len(FRONT_PLAN_FIELDS):] == words
    return dict(plan=dict(zip(FRONT_PLAN_FIELDS, list(info))), tables=dict(zip(FRONT_TABLES, tabs)))


def ntt_config(**kw):
    c = lib().mbls_default_ntt_config()
    for k, v in kw.items():
        if k == "stream":
            c.stream = _stream_handle(v)
        elif k == "coset_gen":
            for i in range(4):
                c.coset_gen.limbs[i] = int(v[i])
        else:
            setattr(c, k, v)
    return c


def vec_config(**kw):
    c = lib().mbls_default_vec_ops_config()
    for k, v in kw.items():
        if k == "stream":
            c.stream = _stream_handle(v)
        else:
            setattr(c, k, v)
    return c


# ----------------------------------------------------------------------------- vecops
_VEC = {"add": "bls12_381_vector_add", "sub": "bls12_381_vector_sub", "mul": "bls12_381_vector_mul",
        "scalar_mul": "bls12_381_scalar_mul_vec", "scalar_add": "bls12_381_scalar_add_vec"}


def vec_op(op, a, b, out=None, stream=None, is_async=False, batch=1, columns_batch=False):
    """a, b: (batch*n,4) uint64 numpy (host) or torch (device) arrays; for scalar ops `a`
    holds one element per batch member (host numpy unless it is a device tensor)."""
    total = b.shape[0]
    if out is None:
        out = np.zeros((total, 4), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=_is_dev(a), is_b_on_device=_is_dev(b), is_result_on_device=_is_dev(out),
                     is_async=is_async, stream=stream, batch_size=batch, columns_batch=columns_batch)
    check(getattr(lib(), _VEC[op])(_p(a), _p(b), total // batch, ctypes.byref(cfg), _p(out)), _VEC[op])
    return out


# ----------------------------------------------------------------------------- point forms
_CONV = {("g1", "to_projective"): ("bls12_381_g1_affine_to_projective", 18),
         ("g1", "to_affine"): ("bls12_381_g1_projective_to_affine", 12),
         ("g2", "to_affine"): ("bls12_381_g2_projective_to_affine", 24)}


def convert_points(group, direction, pts, out=None, stream=None, is_async=False):
    """Batch point-form conversion (reference point_ops.cu:759,844,924): `pts` is (n, k) uint64
    (numpy host or torch device), Montgomery; returns (n, k') in the other form."""
    name, words = _CONV[(group, direction)]
    n = pts.shape[0]
    if out is None:
        out = np.zeros((n, words), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=_is_dev(pts), is_result_on_device=_is_dev(out), stream=stream, is_async=is_async)
    check(getattr(lib(), name)(_p(pts), n, ctypes.byref(cfg), _p(out)), name)
    return out


def scalar_mul(group, bases, scalars, *, scalars_mont=False, out=None, stream=None, is_async=False):
    """Batch scalar multiplication out[i] = scalars[i] * bases[i] (mbls_g*_scalar_mul): `bases`
    (n, 12 | 24) uint64 Montgomery affine, `scalars` (n, 4) uint64, standard form unless
    scalars_mont; each numpy (host) or torch (device).  Returns (n, 18 | 36) Jacobian Montgomery
    (identity Z = 0), host numpy unless `out` is a device tensor; convert_points(group,
    "to_affine", ...) gives affine points.  Bases are assumed to lie in the order-r subgroup
    (check_points establishes it)."""
    n = bases.shape[0]
    assert scalars.shape[0] == n
    if out is None:
        out = np.zeros((n, 18 if group == "g1" else 36), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=_is_dev(bases), is_b_on_device=_is_dev(scalars), is_result_on_device=_is_dev(out),
                     stream=stream, is_async=is_async)
    name = "mbls_g1_scalar_mul" if group == "g1" else "mbls_g2_scalar_mul"
    check(getattr(lib(), name)(_p(bases), _p(scalars), n, bool(scalars_mont), ctypes.byref(cfg), _p(out)), name)
    return out


# mbls_point_status (include/bls12_381_mi355x.h): 0 and 1 are valid, >= 2 invalid
POINT_OK, POINT_IDENTITY, POINT_NONCANONICAL, POINT_OFF_CURVE, POINT_OFF_SUBGROUP = range(5)


def check_points(group, pts, *, points_mont=True, out=None, count=True, stream=None, is_async=False):
    """Batch point validation (mbls_g*_check_points): `pts` (n, 12 | 24) uint64 affine, Montgomery
    unless points_mont is False, numpy (host) or torch (device).  Returns (status, n_invalid):
    status[i] is the first failing test of point i (POINT_*), a host uint8 array, or `out` when it
    is a device uint8 tensor, or None for out=False (count only); n_invalid is the number of
    statuses >= 2, or None for count=False (then a device `out` with is_async does not wait)."""
    n = pts.shape[0]
    if out is None:
        out = np.zeros(n, dtype=np.uint8)
    elif out is False:
        out = None
    cnt = ctypes.c_uint64(0) if count else None
    cfg = vec_config(is_a_on_device=_is_dev(pts), is_result_on_device=_is_dev(out), stream=stream, is_async=is_async)
    name = "mbls_g1_check_points" if group == "g1" else "mbls_g2_check_points"
    check(getattr(lib(), name)(_p(pts), n, bool(points_mont), ctypes.byref(cfg), _p(out),
                               ctypes.byref(cnt) if count else None), name)
    return out, (int(cnt.value) if count else None)


# mbls_decode_status (include/bls12_381_mi355x.h): 0 and 1 are valid, >= 2 invalid; 0..3 line up with
# POINT_*, 4 (POINT_OFF_SUBGROUP) is left unused
DECODE_OK, DECODE_IDENTITY, DECODE_NONCANONICAL, DECODE_NO_POINT, DECODE_BAD_FLAGS = 0, 1, 2, 3, 5


def decompress_points(group, data, *, points_mont=True, out=None, status=None, count=True, stream=None,
                      is_async=False):
    """Batch point decompression (mbls_g*_decompress): `data` (n, 48 | 96) uint8 records in the ZCash
    compressed encoding, numpy (host) or torch (device).  Returns (points, status, n_invalid): points
    (n, 12 | 24) uint64 affine, Montgomery unless points_mont is False, all-zero for every record
    whose status is not DECODE_OK; status[i] the first failing test of record i (DECODE_*);
    n_invalid the number of statuses >= 2, or None for count=False.  Points and status are host
    numpy arrays by default; `out` (int64 torch) and `status` (uint8 torch) place them, together, on
    the device (then a call with count=False and is_async does not wait); status=False asks for
    none.  No subgroup test is made: check_points on the result is the next step."""
    n, nl = data.shape[0], 12 if group == "g1" else 24
    assert data.shape[1] == 4 * nl
    if status is False:
        status = None
    elif status is None:
        if _is_dev(out):
            import torch
            status = torch.zeros((n,), dtype=torch.uint8, device=out.device)
        else:
            status = np.zeros(n, dtype=np.uint8)
    if out is None:
        out = torch_u64((n, nl), device=status.device) if _is_dev(status) else np.zeros((n, nl), dtype=np.uint64)
    assert status is None or _is_dev(status) == _is_dev(out), "points and status share one placement"
    cnt = ctypes.c_uint64(0) if count else None
    cfg = vec_config(is_a_on_device=_is_dev(data), is_result_on_device=_is_dev(out), stream=stream, is_async=is_async)
    name = "mbls_g1_decompress" if group == "g1" else "mbls_g2_decompress"
    check(getattr(lib(), name)(_p(data), n, bool(points_mont), ctypes.byref(cfg), _p(out), _p(status),
                               ctypes.byref(cnt) if count else None), name)
    return out, status, (int(cnt.value) if count else None)


def compress_points(group, pts, *, points_mont=True, out=None, stream=None, is_async=False):
    """Batch point compression (mbls_g*_compress): `pts` (n, 12 | 24) uint64 affine, Montgomery unless
    points_mont is False, numpy (host) or torch (device); the all-zero point gives the infinity
    record.  Returns (n, 48 | 96) uint8, host numpy unless `out` is a device uint8 tensor.  Nothing
    is validated."""
    n = pts.shape[0]
    if out is None:
        out = np.zeros((n, 48 if group == "g1" else 96), dtype=np.uint8)
    cfg = vec_config(is_a_on_device=_is_dev(pts), is_result_on_device=_is_dev(out), stream=stream, is_async=is_async)
    name = "mbls_g1_compress" if group == "g1" else "mbls_g2_compress"
    check(getattr(lib(), name)(_p(pts), n, bool(points_mont), ctypes.byref(cfg), _p(out)), name)
    return out


def vec_sum(x, out=None, stream=None):
    """sum of the device tensor x (n,4) -> (1,4) numpy (host) unless `out` is a device tensor"""
    if out is None:
        out = np.zeros((1, 4), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=True, is_b_on_device=True, is_result_on_device=_is_dev(out), stream=stream)
    check(lib().vec_sum_cuda(_p(out), _p(x), x.shape[0], ctypes.byref(cfg)), "vec_sum_cuda")
    return out


def vector_sum(a, batch=1, out=None, stream=None, is_async=False):
    """ICICLE vector_sum (bls12_381_vector_sum): `batch` row-major sums of a (batch*n, 4), host
    numpy or device torch -> (batch, 4) numpy unless `out` is a device tensor"""
    if out is None:
        out = np.zeros((batch, 4), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=_is_dev(a), is_b_on_device=True, is_result_on_device=_is_dev(out),
                     stream=stream, batch_size=batch, is_async=is_async)
    check(lib().bls12_381_vector_sum(_p(a), a.shape[0] // batch, ctypes.byref(cfg), _p(out)), "bls12_381_vector_sum")
    return out


def batch_inv(x, out, stream=None):
    """element-wise inverses of device tensor x into device tensor out (may be x)"""
    cfg = vec_config(stream=stream)
    check(lib().bls12_381_batch_inv_cuda(_p(out), _p(x), x.shape[0], ctypes.byref(cfg)), "bls12_381_batch_inv_cuda")
    return out


# ----------------------------------------------------------------------------- scans
GEOMETRY_FIELDS = ("K", "tile", "groups", "span")


def scan_geometry(n):
    """the launch geometry of the scans for a member of n elements (mbls_fr_scan_geometry; host
    only): dict of GEOMETRY_FIELDS -- elements per thread, elements per tile, workgroups, elements
    per workgroup span"""
    out = (ctypes.c_int32 * len(GEOMETRY_FIELDS))()
    check(lib().mbls_fr_scan_geometry(n, out), "mbls_fr_scan_geometry")
    return dict(zip(GEOMETRY_FIELDS, list(out)))


def _like(ref, rows):
    """(rows, 4) uint64 storage placed as `ref` is: a device tensor or a host array"""
    return torch_u64((rows, 4), device=ref.device) if _is_dev(ref) else np.zeros((rows, 4), dtype=np.uint64)


def prefix_product(num, den=None, *, init=None, inclusive=False, batch=1, out=None, total=False, stream=None,
                   is_async=False):
    """Grand product (mbls_fr_prefix_product): out[i] = init * prod_{j < i} num[j] / den[j] per batch
    member (inclusive: j <= i), 1 / 0 = 0.  num, den (batch*n, 4) uint64 Montgomery, both numpy
    (host) or both torch (device); init (batch, 4), default Montgomery one.  Returns out, a host
    array unless `out` is a device tensor (`out` may be num or den); with total=True, or a
    (batch, 4) buffer placed as `out`, returns (out, total), total[k] = init[k] * all of member k."""
    n = num.shape[0] // batch
    assert den is None or _is_dev(den) == _is_dev(num), "num and den share one placement"
    if out is None:
        out = np.zeros((num.shape[0], 4), dtype=np.uint64)
    if total is True:
        total = _like(out, batch)
    elif total is False:
        total = None
    assert total is None or _is_dev(total) == _is_dev(out), "out and total share one placement"
    cfg = vec_config(is_a_on_device=_is_dev(num), is_b_on_device=_is_dev(init), is_result_on_device=_is_dev(out),
                     is_async=is_async, stream=stream, batch_size=batch)
    check(lib().mbls_fr_prefix_product(_p(num), _p(den), n, _p(init), bool(inclusive), ctypes.byref(cfg), _p(out),
                                       _p(total)), "mbls_fr_prefix_product")
    return out if total is None else (out, total)


def poly_divide_linear(coeffs, z, *, batch=1, out=None, quotient=True, eval=True, stream=None, is_async=False):
    """Division by X - z with remainder (mbls_fr_poly_divide_linear): per batch member p = q * (X - z)
    + p(z).  coeffs (batch*n, 4) uint64 Montgomery, lowest degree first, z (batch, 4), each numpy
    (host) or torch (device).  Returns (q, p_z): q (batch*n, 4) with q[n-1] = 0, `out` when given
    (`out` may be coeffs), None for quotient=False (pure evaluation, no vector is written); p_z
    (batch, 4), `eval` when it is a buffer, None for eval=False.  Both are placed alike: on the
    device when `out` (or, without a quotient, `eval`) is a device tensor, else on the host."""
    n = coeffs.shape[0] // batch
    if not quotient:
        out = None
    elif out is None:
        out = _like(None if isinstance(eval, bool) else eval, coeffs.shape[0])
    if eval is True:
        eval = _like(out, batch) if out is not None else np.zeros((batch, 4), dtype=np.uint64)
    elif eval is False:
        eval = None
    assert out is None or eval is None or _is_dev(out) == _is_dev(eval), "quotient and eval share one placement"
    cfg = vec_config(is_a_on_device=_is_dev(coeffs), is_b_on_device=_is_dev(z),
                     is_result_on_device=_is_dev(out if out is not None else eval), is_async=is_async, stream=stream,
                     batch_size=batch)
    check(lib().mbls_fr_poly_divide_linear(_p(coeffs), n, _p(z), ctypes.byref(cfg), _p(out), _p(eval)),
          "mbls_fr_poly_divide_linear")
    return out, eval


# ----------------------------------------------------------------------------- sort and lookup
SORT_PLAN_FIELDS = ("bits", "passes", "tile", "groups", "sort_bytes", "lookup_bytes")


def sort_plan(n, batch=1):
    """the geometry and scratch of fr_sort / lookup_permute for `batch` members of n elements
    (mbls_fr_sort_plan; host only): dict of SORT_PLAN_FIELDS -- bits per digit, digit passes when no
    key word is skipped, elements per workgroup tile, workgroups per pass, scratch bytes of the sort
    and of the lookup"""
    out = (ctypes.c_int64 * len(SORT_PLAN_FIELDS))()
    check(lib().mbls_fr_sort_plan(n, batch, out), "mbls_fr_sort_plan")
    return dict(zip(SORT_PLAN_FIELDS, list(out)))


def _u32_like(ref, rows):
    if _is_dev(ref):
        import torch
        return torch.zeros((rows,), dtype=torch.int32, device=ref.device)
    return np.zeros(rows, dtype=np.uint32)


def fr_sort(x, *, mont=True, batch=1, perm=False, out=None, stream=None, is_async=False):
    """Stable sort by standard-form value (mbls_fr_sort): x (batch*n, 4) uint64, Montgomery unless
    mont is False, numpy (host) or torch (device); each of the `batch` members is sorted on its own.
    Returns the sorted elements (x's own, moved): `out` when given, else placed as x is; out=False
    asks for none.  With perm=True, or a (batch*n,) uint32 numpy / int32 torch buffer placed as
    `out`, returns (sorted, perm), perm[k*n + i] = the index within member k of its i-th smallest
    element, equal elements in ascending index."""
    n = x.shape[0] // batch
    if out is None:
        out = _like(x, x.shape[0])
    elif out is False:
        out = None
    if perm is True:
        perm = _u32_like(out if out is not None else x, x.shape[0])
    elif perm is False:
        perm = None
    assert out is None or perm is None or _is_dev(out) == _is_dev(perm), "sorted and perm share one placement"
    cfg = vec_config(is_a_on_device=_is_dev(x), is_result_on_device=_is_dev(out if out is not None else perm),
                     is_async=is_async, stream=stream, batch_size=batch)
    check(lib().mbls_fr_sort(_p(x), n, bool(mont), ctypes.byref(cfg), _p(out), _p(perm)), "mbls_fr_sort")
    return out if perm is None else (out, perm)


def lookup_permute(input, table, *, mont=True, batch=1, count=True, out=None, stream=None, is_async=False):
    """The lookup argument's permuted pair (mbls_fr_lookup_permute): input, table (batch*n, 4) uint64,
    Montgomery unless mont is False, both numpy (host) or both torch (device).  Returns
    (permuted_input, permuted_table, n_missing): A' = the sorted input and S' = the table laid out
    beside it as permute_expression_pair does, `out` = (A', S') buffers when given, else placed as
    the input is; n_missing a list of `batch` counts of distinct input values absent from the table
    (any non-zero: a failed lookup), or None for count=False (then device outputs with is_async do
    not wait)."""
    n = input.shape[0] // batch
    assert table.shape[0] == input.shape[0] and _is_dev(table) == _is_dev(input), "input and table share size and placement"
    pin, ptab = out if out is not None else (_like(input, input.shape[0]), _like(input, input.shape[0]))
    assert _is_dev(pin) == _is_dev(ptab), "the outputs share one placement"
    cnt = (ctypes.c_uint64 * batch)() if count else None
    cfg = vec_config(is_a_on_device=_is_dev(input), is_result_on_device=_is_dev(pin), is_async=is_async, stream=stream,
                     batch_size=batch)
    check(lib().mbls_fr_lookup_permute(_p(input), _p(table), n, bool(mont), ctypes.byref(cfg), _p(pin), _p(ptab), cnt),
          "mbls_fr_lookup_permute")
    return pin, ptab, ([int(v) for v in cnt] if count else None)


# ----------------------------------------------------------------------------- log-derivative lookup
def _pointer_table(cols, like=None, what="the operands of a table share one size and placement"):
    """(table, n, on_device) of a list of operands of one size and one placement, `like`'s when given"""
    like = cols[0] if like is None else like
    n, on_dev = like.shape[0], _is_dev(like)
    assert all(c.shape[0] == n and _is_dev(c) == on_dev for c in cols), what
    return (ctypes.c_void_p * len(cols))(*[_p(c) for c in cols]), n, on_dev


def lookup_multiplicities(inputs, table, credit="first", montgomery=True, *, batch=1, count=True, out=None, stream=None,
                          is_async=False):
    """The log-derivative lookup's multiplicity column (mbls_fr_lookup_multiplicities).  inputs: a
    list of 1..64 columns, table: (batch*n, 4) uint64, Montgomery unless montgomery is False, all
    numpy (host) or all torch (device).  Returns (m, n_missing): m[j] = the input cells equal to
    table[j] as a field element in the inputs' form if j is the credited row of its value -- the
    lowest row holding it, credit="last": the highest -- else zero; `out` when given, else placed as
    the table is.  n_missing: a list of `batch` counts of cells whose value the table lacks, or None
    for count=False (then a device output with is_async does not wait)."""
    assert credit in ("first", "last")
    n = table.shape[0] // batch
    cols, _, _ = _pointer_table(inputs, table, "columns and table share one size and placement")
    if out is None:
        out = _like(table, table.shape[0])
    cnt = (ctypes.c_uint64 * batch)() if count else None
    cfg = vec_config(is_a_on_device=_is_dev(table), is_result_on_device=_is_dev(out), is_async=is_async, stream=stream,
                     batch_size=batch)
    check(lib().mbls_fr_lookup_multiplicities(cols, len(inputs), _p(table), n, bool(montgomery), credit == "last",
                                              ctypes.byref(cfg), _p(out), cnt), "mbls_fr_lookup_multiplicities")
    return out, ([int(v) for v in cnt] if count else None)


def prefix_sum(col, init=None, inclusive=False, out=None, total=False, *, batch=1, stream=None, is_async=False):
    """Running sum (mbls_fr_prefix_sum): out[i] = init + sum_{j < i} col[j] per batch member
    (inclusive: j <= i).  col (batch*n, 4) uint64, numpy (host) or torch (device); init (batch, 4),
    default zero.  Returns out, a host array unless `out` is a device tensor (`out` may be col);
    with total=True, or a (batch, 4) buffer placed as `out`, returns (out, total)."""
    n = col.shape[0] // batch
    if out is None:
        out = np.zeros((col.shape[0], 4), dtype=np.uint64)
    if total is True:
        total = _like(out, batch)
    elif total is False:
        total = None
    assert total is None or _is_dev(total) == _is_dev(out), "out and total share one placement"
    cfg = vec_config(is_a_on_device=_is_dev(col), is_b_on_device=_is_dev(init), is_result_on_device=_is_dev(out),
                     is_async=is_async, stream=stream, batch_size=batch)
    check(lib().mbls_fr_prefix_sum(_p(col), n, _p(init), bool(inclusive), ctypes.byref(cfg), _p(out), _p(total)),
          "mbls_fr_prefix_sum")
    return out if total is None else (out, total)


def logup_sum(inputs, table, m, beta, init=None, out=None, total=False, *, batch=1, stream=None, is_async=False):
    """The log-derivative lookup's running sum (mbls_fr_logup_sum): phi[0] = init, phi[i+1] = phi[i] +
    sum_c 1 / (inputs[c][i] + beta) - m[i] / (table[i] + beta), 1 / 0 = 0.  inputs, table, m:
    (batch*n, 4) uint64 Montgomery, all numpy (host) or all torch (device); beta, init (batch, 4),
    placed alike, init default zero.  Returns phi[0 .. n): `out` when given (it may be m), else a host
    array; with total=True, or a (batch, 4) buffer placed as `out`, returns (out, total), total =
    phi[n], zero for a satisfied lookup started from zero."""
    n = table.shape[0] // batch
    cols, _, _ = _pointer_table(inputs, table, "columns and table share one size and placement")
    assert m.shape[0] == table.shape[0] and _is_dev(m) == _is_dev(table), "m is sized and placed as the table is"
    assert init is None or _is_dev(init) == _is_dev(beta), "beta and init share one placement"
    if out is None:
        out = np.zeros((table.shape[0], 4), dtype=np.uint64)
    if total is True:
        total = _like(out, batch)
    elif total is False:
        total = None
    assert total is None or _is_dev(total) == _is_dev(out), "out and total share one placement"
    cfg = vec_config(is_a_on_device=_is_dev(table), is_b_on_device=_is_dev(beta), is_result_on_device=_is_dev(out),
                     is_async=is_async, stream=stream, batch_size=batch)
    check(lib().mbls_fr_logup_sum(cols, len(inputs), _p(table), _p(m), n, _p(beta), _p(init), ctypes.byref(cfg), _p(out),
                                  _p(total)), "mbls_fr_logup_sum")
    return out if total is None else (out, total)


# ----------------------------------------------------------------------------- inner products
INNER_PLAN_FIELDS = ("tile", "defer", "CB", "VB", "max_workgroups", "group_cap", "tiles_per_group", "groups",
                     "workgroups", "inner_bytes", "multi_eval_bytes", "pow_log")


def inner_plan(n, n_columns=1, n_vectors=1):
    """the geometry and scratch of inner_products / multi_eval for n rows (mbls_fr_inner_plan; host
    only): dict of INNER_PLAN_FIELDS -- rows per tile, products deferred per reduction, columns and
    vectors per block, the most workgroups of any call, the most row groups of these counts (a
    workgroup takes several tiles only above group_cap * tile rows), tiles per workgroup, row groups,
    workgroups launched, scratch bytes of inner_products and of multi_eval, the power tables' split"""
    out = (ctypes.c_int64 * len(INNER_PLAN_FIELDS))()
    check(lib().mbls_fr_inner_plan(n, n_columns, n_vectors, out), "mbls_fr_inner_plan")
    return dict(zip(INNER_PLAN_FIELDS, list(out)))


def inner_products(columns, vectors, *, out=None, stream=None, is_async=False):
    """out[p * len(vectors) + k] = sum_i columns[p][i] * vectors[k][i] (mbls_fr_inner_products).
    columns: a list of 1..1024 (n, 4) uint64 Montgomery columns, all numpy (host) or all torch
    (device); vectors: a list of 1..16 such, placed alike among themselves.  Returns out,
    (len(columns) * len(vectors), 4): `out` when given, else placed as the columns are."""
    ctab, n, c_dev = _pointer_table(columns)
    vtab, nv, v_dev = _pointer_table(vectors)
    assert n == nv, "columns and vectors share one size"
    if out is None:
        out = _like(columns[0], len(columns) * len(vectors))
    cfg = vec_config(is_a_on_device=c_dev, is_b_on_device=v_dev, is_result_on_device=_is_dev(out), is_async=is_async,
                     stream=stream)
    check(lib().mbls_fr_inner_products(ctab, len(columns), vtab, len(vectors), n, ctypes.byref(cfg), _p(out)),
          "mbls_fr_inner_products")
    return out


def multi_eval(columns, points, *, out=None, stream=None, is_async=False):
    """out[p * k_points + k] = columns[p] as a polynomial, lowest degree first, at points[k]
    (mbls_fr_multi_eval).  columns: a list of 1..1024 (n, 4) uint64 Montgomery columns, all numpy or all
    torch; points (1..16, 4), numpy or torch.  Returns out, (len(columns) * k_points, 4): `out` when
    given, else placed as the columns are."""
    ctab, n, c_dev = _pointer_table(columns)
    if out is None:
        out = _like(columns[0], len(columns) * points.shape[0])
    cfg = vec_config(is_a_on_device=c_dev, is_b_on_device=_is_dev(points), is_result_on_device=_is_dev(out),
                     is_async=is_async, stream=stream)
    check(lib().mbls_fr_multi_eval(ctab, len(columns), n, _p(points), points.shape[0], ctypes.byref(cfg), _p(out)),
          "mbls_fr_multi_eval")
    return out


def powers(base, n, *, init=None, out=None, stream=None, is_async=False):
    """out[k * n + i] = init[k] * base[k]^i (mbls_fr_powers), x^0 = 1 also for x = 0.  base (batch, 4)
    uint64 Montgomery, init likewise and placed as base is, default Montgomery one.  Returns out,
    (batch * n, 4): `out` when given, else placed as base is."""
    batch = base.shape[0]
    assert init is None or (init.shape[0] == batch and _is_dev(init) == _is_dev(base)), "base and init share shape and placement"
    if out is None:
        out = _like(base, batch * n)
    cfg = vec_config(is_b_on_device=_is_dev(base), is_result_on_device=_is_dev(out), is_async=is_async, stream=stream,
                     batch_size=batch)
    check(lib().mbls_fr_powers(_p(base), _p(init), n, ctypes.byref(cfg), _p(out)), "mbls_fr_powers")
    return out


# ----------------------------------------------------------------------------- expression evaluator
(EXPR_COLUMN, EXPR_CONST, EXPR_ADD, EXPR_SUB, EXPR_MUL, EXPR_NEG, EXPR_DOUBLE, EXPR_SQUARE, EXPR_SCALE, EXPR_HORNER,
 EXPR_EMIT) = range(11)
EXPR_CHECK_FIELDS = ("depth", "loads", "muls", "pairs")


class ExprOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("a", ctypes.c_int32), ("b", ctypes.c_int32)]


def _expr_program(program):
    ops = (ExprOp * max(len(program), 1))()
    for k, (op, a, b) in enumerate(program):
        ops[k].op, ops[k].a, ops[k].b = int(op), int(a), int(b)
    return ops


def expr_check(program, n_columns, n_constants, n_outputs):
    """validate and describe a program of (op, a, b) tuples (mbls_fr_expr_check; host only): dict of
    EXPR_CHECK_FIELDS -- maximum stack depth, COLUMN loads per row, field multiplications per row,
    distinct (column, rotation) pairs.  Raises IcicleError(INVALID_ARGUMENT) for a malformed one."""
    out = (ctypes.c_int32 * len(EXPR_CHECK_FIELDS))()
    check(lib().mbls_fr_expr_check(_expr_program(program), len(program), n_columns, n_constants, n_outputs, out),
          "mbls_fr_expr_check")
    return dict(zip(EXPR_CHECK_FIELDS, list(out)))


def _eval_rows(entry, name, ops, n_ops, columns, constants, n_outputs, rot_stride, out, stream, is_async):
    """the body eval_program and eval_graph share: `entry` over `ops`, the program in its C form"""
    table, n, on_dev = _pointer_table(columns, what="columns share one size and placement")
    if out is None:
        out = _like(columns[0], n_outputs * n)
    cfg = vec_config(is_a_on_device=on_dev, is_b_on_device=_is_dev(constants), is_result_on_device=_is_dev(out),
                     is_async=is_async, stream=stream)
    check(entry(table, len(columns), n, rot_stride, _p(constants), 0 if constants is None else constants.shape[0], ops,
                n_ops, n_outputs, ctypes.byref(cfg), _p(out)), name)
    return out


def eval_program(columns, program, *, constants=None, n_outputs=1, rot_stride=1, out=None, stream=None, is_async=False):
    """Run `program`, a list of (op, a, b) tuples of EXPR_* opcodes, once per row (mbls_fr_eval_program).
    columns: a list of (n, 4) uint64 Montgomery columns, all numpy (host) or all torch (device);
    COLUMN a, b reads columns[a][(i + b * rot_stride) mod n].  constants (k, 4), numpy or torch.
    Returns out, (n_outputs * n, 4) with output k at rows k * n .. (k + 1) * n: `out` when given (it may
    overlap no column), else placed as the columns are."""
    return _eval_rows(lib().mbls_fr_eval_program, "mbls_fr_eval_program", _expr_program(program), len(program), columns,
                      constants, n_outputs, rot_stride, out, stream, is_async)


# ----------------------------------------------------------------------------- graph evaluator
(GRAPH_ADD, GRAPH_SUB, GRAPH_MUL, GRAPH_SQUARE, GRAPH_DOUBLE, GRAPH_NEG, GRAPH_HORNER, GRAPH_STORE,
 GRAPH_EMIT) = range(9)
(GRAPH_NONE, GRAPH_VALUE, GRAPH_COLUMN, GRAPH_CONST) = range(4)
GRAPH_CHECK_FIELDS = ("peak", "peak_at", "resident", "forwarded", "loads", "pairs", "muls", "budget")


class GraphSrc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("idx", ctypes.c_int32), ("rot", ctypes.c_int32)]


class GraphOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("a", GraphSrc), ("b", GraphSrc), ("c", ctypes.c_int32)]


def _graph_program(program):
    """(op, a, b, c) tuples, a and b (kind, idx, rot) triples, as one contiguous GraphOp array"""
    flat = np.array([(op, *a, *b, c) for op, a, b, c in program], dtype=np.int32).reshape(-1, 8)
    ops = (GraphOp * max(len(program), 1))()
    ctypes.memmove(ops, flat.ctypes.data, flat.nbytes)
    return ops


def graph_check(program, n_columns, n_constants, n_outputs):
    """validate and describe a graph program (mbls_fr_graph_check; host only): dict of
    GRAPH_CHECK_FIELDS -- the peak of resident values, the first op at which it is reached, resident
    values, forwarded operands, column loads and products per row, distinct (column, rot) pairs, the
    budget.  Raises IcicleError(INVALID_ARGUMENT) for a malformed one; when only the peak is at fault
    the error carries the same dict as `info`."""
    out = (ctypes.c_int32 * len(GRAPH_CHECK_FIELDS))(*([-1] * len(GRAPH_CHECK_FIELDS)))
    code = lib().mbls_fr_graph_check(_graph_program(program), len(program), n_columns, n_constants, n_outputs, out)
    info = dict(zip(GRAPH_CHECK_FIELDS, list(out)))
    if code != SUCCESS:
        err = IcicleError(code, "mbls_fr_graph_check")
        if out[0] >= 0:
            err.info = info
        raise err
    return info


def eval_graph(columns, program, *, constants=None, n_outputs=1, rot_stride=1, out=None, stream=None, is_async=False):
    """Run `program`, a list of (op, a, b, c) tuples of GRAPH_* opcodes whose a and b are (kind, idx, rot)
    sources, once per row (mbls_fr_eval_graph); op k defines value k.  columns, constants, out and the
    result are as eval_program's."""
    return _eval_rows(lib().mbls_fr_eval_graph, "mbls_fr_eval_graph", _graph_program(program), len(program), columns,
                      constants, n_outputs, rot_stride, out, stream, is_async)


# ----------------------------------------------------------------------------- NTT
def ntt_init_domain(root_mont=None):
    if root_mont is None:  # canonical 2^32-th root, Montgomery form
        root_mont = np.array([0xb9b58d8c5f0e466a, 0x5b1b4c801819d7ec, 0x0af53ae352a31e64, 0x5bf3adda19e9b27b],
                             dtype=np.uint64)
    cfg = NTTInitDomainConfig()
    check(lib().bls12_381_ntt_init_domain_cuda(_p(np.ascontiguousarray(root_mont, dtype=np.uint64)),
                                               ctypes.byref(cfg)), "ntt_init_domain")


ORDERINGS = {"NN": 0, "NR": 1, "RN": 2, "RR": 3, "NM": 4, "MN": 5}


def ntt(x, inverse=False, out=None, batch=1, stream=None, is_async=False, coset_gen=None, ordering="NN",
        columns_batch=False, entry="ntt"):
    """x: (batch*n, 4) uint64 numpy (host) or torch (device).  entry: the exported symbol that takes
    the call -- "ntt" (bls12_381_ntt_cuda), "field" (bls12_381_field_ntt_cuda), both with the coset
    generator in the config, or "coset" (bls12_381_coset_ntt_cuda: the generator as an argument,
    the config's left at its default)."""
    total = x.shape[0]
    n = total // batch
    if out is None:
        out = np.zeros((total, 4), dtype=np.uint64) if isinstance(x, np.ndarray) else None
    kw = dict(batch_size=batch, are_inputs_on_device=_is_dev(x), are_outputs_on_device=_is_dev(out),
              is_async=is_async, stream=stream, ordering=ORDERINGS[ordering], columns_batch=columns_batch)
    if coset_gen is not None and entry != "coset":
        kw["coset_gen"] = coset_gen
    cfg = ntt_config(**kw)
    d = 1 if inverse else 0
    if entry == "coset":
        g = FrC()
        for i in range(4):
            g.limbs[i] = int(cfg.coset_gen.limbs[i] if coset_gen is None else coset_gen[i])
        check(lib().bls12_381_coset_ntt_cuda(_p(x), n, d, ctypes.byref(g), ctypes.byref(cfg), _p(out)), "coset_ntt")
    else:
        fn = {"ntt": lib().bls12_381_ntt_cuda, "field": lib().bls12_381_field_ntt_cuda}[entry]
        check(fn(_p(x), n, d, ctypes.byref(cfg), _p(out)), entry)
    return out


def _coset_arg(coset_gen):
    """a host FrC holding the generator's four limbs, or None"""
    if coset_gen is None:
        return None
    g = FrC()
    for i in range(4):
        g.limbs[i] = int(coset_gen[i])
    return ctypes.byref(g)


def coeff_to_extended(coeffs, extended_size, coset_gen=None, out=None, stream=None, batch=1, is_async=False):
    """halo2's coeff_to_extended (mbls_fr_coeff_to_extended): coeffs (batch*size, 4) uint64 Montgomery,
    size any value in 1..extended_size, numpy (host) or torch (device) -> the polynomial's values on
    g * H_extended_size, (batch*extended_size, 4).  coset_gen: four Montgomery limbs (host), None for
    no coset.  Returns `out` when given (it may not overlap coeffs), else storage placed as coeffs is."""
    size = coeffs.shape[0] // batch
    if out is None:
        out = _like(coeffs, batch * extended_size)
    cfg = ntt_config(batch_size=batch, are_inputs_on_device=_is_dev(coeffs), are_outputs_on_device=_is_dev(out),
                     is_async=is_async, stream=stream)
    check(lib().mbls_fr_coeff_to_extended(_p(coeffs), size, extended_size, _coset_arg(coset_gen), ctypes.byref(cfg),
                                          _p(out)), "mbls_fr_coeff_to_extended")
    return out


def extended_to_coeff(evals, out_size, coset_gen=None, vanishing_inv=None, out=None, stream=None, batch=1,
                      is_async=False):
    """halo2's divide_by_vanishing_poly + extended_to_coeff + truncation (mbls_fr_extended_to_coeff):
    evals (batch*extended_size, 4) uint64 Montgomery values on g * H_extended_size, numpy (host) or
    torch (device); vanishing_inv (period, 4), placed as evals is, multiplies evals[j] by entry
    j mod period first (None: no division).  Returns the first out_size coefficients of each member,
    (batch*out_size, 4): `out` when given (it may not overlap evals), else placed as evals is.  The same
    coset_gen as in coeff_to_extended undoes its coset."""
    n = evals.shape[0] // batch
    assert vanishing_inv is None or _is_dev(vanishing_inv) == _is_dev(evals), "evals and vanishing_inv share one placement"
    if out is None:
        out = _like(evals, batch * out_size)
    cfg = ntt_config(batch_size=batch, are_inputs_on_device=_is_dev(evals), are_outputs_on_device=_is_dev(out),
                     is_async=is_async, stream=stream)
    period = 0 if vanishing_inv is None else vanishing_inv.shape[0]
    check(lib().mbls_fr_extended_to_coeff(_p(evals), n, out_size, _coset_arg(coset_gen), _p(vanishing_inv), period,
                                          ctypes.byref(cfg), _p(out)), "mbls_fr_extended_to_coeff")
    return out


DOMAIN_PLAN_FIELDS = ("passes", "E", "skipped", "rows", "fwd_scratch", "inv_scratch")


def domain_plan(size, extended_size):
    """what coeff_to_extended / extended_to_coeff do for (size, extended_size) (mbls_fr_domain_plan;
    host only): dict of DOMAIN_PLAN_FIELDS -- passes, extension bits E, DIT stages skipped as
    replication, input rows the first pass reads per tile, scratch elements per member of the forward
    and of the inverse call -- plus plan = [(s0, L, logC)] per pass, the NTT's own"""
    out = (ctypes.c_int32 * 18)()
    check(lib().mbls_fr_domain_plan(size, extended_size, out), "mbls_fr_domain_plan")
    d = dict(zip(DOMAIN_PLAN_FIELDS, list(out)))
    d["plan"] = [tuple(out[6 + 3 * p:9 + 3 * p]) for p in range(out[0])]
    return d


def ecntt(points, inverse=False, out=None, stream=None, is_async=False):
    """G1 EC-NTT (mbls_g1_ecntt): `points` (n, 12) uint64 Montgomery affine, n a power of two, numpy
    (host) or torch (device).  forward out_j = sum_i [w^(ij)] P_i, inverse out_i = [n^-1] sum_j
    [w^(-ij)] P_j with the Fr NTT's root w of that size, natural order: the inverse of a monomial
    SRS [s^j] G is the Lagrange SRS.  Returns (n, 12) canonical Montgomery affine, host numpy unless
    `out` is a device tensor (`out` may be `points`).  Points are assumed to lie in the order-r
    subgroup."""
    n = points.shape[0]
    if out is None:
        out = np.zeros((n, 12), dtype=np.uint64)
    cfg = ntt_config(are_inputs_on_device=_is_dev(points), are_outputs_on_device=_is_dev(out), is_async=is_async,
                     stream=stream)
    check(lib().mbls_g1_ecntt(_p(points), n, 1 if inverse else 0, ctypes.byref(cfg), _p(out)), "mbls_g1_ecntt")
    return out


# ----------------------------------------------------------------------------- fixed base
FIXED_BASE_PLAN_FIELDS = ("c", "W", "rows", "entries", "entry_bytes", "block", "chunk", "scratch_per_point")


def fixed_base_plan(group):
    """the geometry of the fixed-base multiplication of `group` (mbls_fixed_base_plan; host only):
    dict of FIXED_BASE_PLAN_FIELDS"""
    out = (ctypes.c_int64 * len(FIXED_BASE_PLAN_FIELDS))()
    check(lib().mbls_fixed_base_plan(1 if group == "g1" else 2, out), "mbls_fixed_base_plan")
    return dict(zip(FIXED_BASE_PLAN_FIELDS, list(out)))


def fixed_base_recode(scalar):
    """the W signed digits of `scalar` mod r (an int below 2^256, standard form), lowest window first,
    by the function the kernels run (mbls_fixed_base_recode; host only)"""
    limbs = np.array([(int(scalar) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    digits = np.zeros(fixed_base_plan("g1")["W"], dtype=np.int32)
    check(lib().mbls_fixed_base_recode(_p(limbs), _p(digits)), "mbls_fixed_base_recode")
    return [int(d) for d in digits]


def fixed_base_table(group, base, stream=None, is_async=False):
    """The table of `base` ((12 | 24,) or (1, 12 | 24) uint64 Montgomery affine, numpy or torch) that
    fixed_base_mul and srs_from_secret take (mbls_g*_fixed_base_table): a device tensor of
    fixed_base_plan(group)["entries"] affine points, entry w * rows + d - 1 = [d 2^(c w)] base.  The
    base is assumed to lie in the order-r subgroup."""
    import torch
    plan = fixed_base_plan(group)
    # empty, not zeros: a fill on torch's current stream could land after the build on `stream`
    table = torch.empty((plan["entries"], plan["entry_bytes"] // 8), dtype=torch.int64, device="cuda")
    cfg = vec_config(is_a_on_device=_is_dev(base), is_result_on_device=True, stream=stream, is_async=is_async)
    name = "mbls_g1_fixed_base_table" if group == "g1" else "mbls_g2_fixed_base_table"
    check(getattr(lib(), name)(_p(base), ctypes.byref(cfg), _p(table)), name)
    return table


def fixed_base_mul(group, table, scalars, *, scalars_mont=False, out=None, stream=None, is_async=False):
    """out[i] = [scalars[i] mod r] base (mbls_g*_fixed_base_mul) for the base of `table`
    (fixed_base_table, a device tensor): `scalars` (n, 4) uint64, standard form unless scalars_mont,
    numpy (host) or torch (device).  Returns (n, 12 | 24) canonical Montgomery affine, identity all
    zero, host numpy unless `out` is a device tensor.  Not constant time."""
    n = scalars.shape[0]
    if out is None:
        out = np.zeros((n, 12 if group == "g1" else 24), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=True, is_b_on_device=_is_dev(scalars), is_result_on_device=_is_dev(out),
                     stream=stream, is_async=is_async)
    name = "mbls_g1_fixed_base_mul" if group == "g1" else "mbls_g2_fixed_base_mul"
    check(getattr(lib(), name)(_p(table), _p(scalars), n, bool(scalars_mont), ctypes.byref(cfg), _p(out)), name)
    return out


def srs_from_secret(table, tau, n, lagrange=False, out=None, stream=None, is_async=False):
    """A KZG SRS of n G1 points from the secret `tau` ((4,) uint64 Montgomery, host numpy) and the
    table of the generator (mbls_g1_srs_from_secret): out[i] = [tau^i] G, or [L_i(tau)] G over the
    Fr NTT's domain of size n = 2^k when `lagrange`.  Returns (n, 12) canonical Montgomery affine,
    host numpy unless `out` is a device tensor.  Not constant time: for unsafe_setup and tests."""
    if out is None:
        out = np.zeros((n, 12), dtype=np.uint64)
    cfg = vec_config(is_a_on_device=True, is_result_on_device=_is_dev(out), stream=stream, is_async=is_async)
    tau = np.ascontiguousarray(tau, dtype=np.uint64)
    check(lib().mbls_g1_srs_from_secret(_p(table), _p(tau), n, 1 if lagrange else 0, ctypes.byref(cfg), _p(out)),
          "mbls_g1_srs_from_secret")
    return out


# ----------------------------------------------------------------------------- MSM
def msm(group, scalars, bases, *, icicle=True, scalars_mont=False, points_mont=True, c=0, bitsize=0,
        precompute_factor=1, batch=1, shared_bases=True, out=None, stream=None, is_async=False, n=None):
    """scalars (batch*n, 4) u64, bases (n*F[*batch], 12|24) u64; host numpy or device torch.
    icicle=True -> ICICLE semantics (standard (x, y, 1)); False -> the reference's raw entry
    (standard scalars, Jacobian Montgomery); "jacobian" -> ICICLE inputs, Jacobian Montgomery
    result (one rank's step of the sharded MSM)."""
    nl = 18 if group == "g1" else 36
    if n is None:
        n = scalars.shape[0] // batch
    if out is None:
        out = np.zeros((batch, nl), dtype=np.uint64)
    cfg = msm_config(c=c, bitsize=bitsize, precompute_factor=precompute_factor, batch_size=batch,
                     are_points_shared_in_batch=shared_bases, are_scalars_on_device=_is_dev(scalars),
                     are_scalars_montgomery_form=scalars_mont, are_points_on_device=_is_dev(bases),
                     are_points_montgomery_form=points_mont, are_results_on_device=_is_dev(out),
                     is_async=is_async, stream=stream)
    if icicle == "jacobian":
        fn = lib().mbls_g1_msm_jacobian if group == "g1" else lib().mbls_g2_msm_jacobian
    elif icicle:
        fn = lib().bls12_381_icicle_g1_msm if group == "g1" else lib().bls12_381_icicle_g2_msm
    else:
        fn = lib().bls12_381_g1_msm_cuda if group == "g1" else lib().bls12_381_g2_msm_cuda
    check(fn(_p(scalars), _p(bases), n, ctypes.byref(cfg), _p(out)), f"{group} msm")
    return out


def precompute_bases(group, bases, factor, n, c=0, out=None, points_mont=True):
    """ICICLE precompute_bases: out[i*factor + f] = 2^(s f) P_i, s = ceil(256 / factor) (the
    shift depends on the factor only, so c is irrelevant); output Montgomery affine."""
    nl = 12 if group == "g1" else 24
    if out is None:
        out = np.zeros((n * factor, nl), dtype=np.uint64)
    cfg = msm_config(precompute_factor=factor, c=c, are_points_on_device=_is_dev(bases),
                     are_points_montgomery_form=points_mont, are_results_on_device=_is_dev(out))
    fn = (lib().bls12_381_icicle_g1_msm_precompute_bases if group == "g1"
          else lib().bls12_381_icicle_g2_msm_precompute_bases)
    check(fn(_p(bases), n, ctypes.byref(cfg), _p(out)), "precompute_bases")
    return out


# ----------------------------------------------------------------------------- utilities
def gen_scalars(out_dev, seed, montgomery=False, stream=None, start=0):
    """elements start .. start + len(out_dev) - 1 of scalar stream `seed`"""
    check(lib().mbls_gen_scalars_range(_p(out_dev), seed, start, out_dev.shape[0], montgomery,
                                       _stream_handle(stream)), "gen_scalars")


def gen_bases(group, out_dev, seed, stream=None, start=0):
    fn = lib().mbls_gen_g1_bases_range if group == "g1" else lib().mbls_gen_g2_bases_range
    check(fn(_p(out_dev), seed, start, out_dev.shape[0], _stream_handle(stream)), "gen_bases")


def msm_multi_device(group, scalars, bases_per_dev, devs, n, *, scalars_mont=True, points_mont=True, out=None,
                     stream=None, is_async=False):
    """mbls_g*_msm_multi_device: shard k of n points runs on devs[k] with bases_per_dev[k] (that
    shard's bases, device tensors); scalars host numpy or device torch (devs[0]); ICICLE (x, y, 1)
    result (host numpy unless `out` is a device tensor on devs[0])"""
    nl = 18 if group == "g1" else 36
    if out is None:
        out = np.zeros((1, nl), dtype=np.uint64)
    k = len(devs)
    ptrs = (ctypes.c_void_p * k)(*[b.data_ptr() for b in bases_per_dev])
    dv = (ctypes.c_int * k)(*devs)
    cfg = msm_config(are_scalars_on_device=_is_dev(scalars), are_scalars_montgomery_form=scalars_mont,
                     are_points_on_device=True, are_points_montgomery_form=points_mont,
                     are_results_on_device=_is_dev(out), is_async=is_async, stream=stream)
    fn = lib().mbls_g1_msm_multi_device if group == "g1" else lib().mbls_g2_msm_multi_device
    check(fn(_p(scalars), ptrs, dv, k, n, ctypes.byref(cfg), _p(out)), f"{group} msm_multi_device")
    return out


def msm_accumulate_event(stream, event):
    """mbls_msm_accumulate_event: the next single MSM on `stream` records the raw hipEvent_t
    `event` (an int handle, or None to clear) when its accumulation is enqueued (its tail starts)"""
    check(lib().mbls_msm_accumulate_event(_stream_handle(stream), ctypes.c_void_p(event) if event else None),
          "mbls_msm_accumulate_event")


class HipEvent:
    """a raw hipEvent_t (timing disabled) that another stream can wait on (hipStreamWaitEvent)"""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        self.hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
        self.hip.hipStreamWaitEvent.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
        self.ev = ctypes.c_void_p()
        if self.hip.hipEventCreateWithFlags(ctypes.byref(self.ev), 2) != 0:  # hipEventDisableTiming
            raise RuntimeError("hipEventCreateWithFlags failed")

    @property
    def handle(self):
        return self.ev.value

    def wait(self, stream):
        """make `stream` (torch stream) wait for the event"""
        if self.hip.hipStreamWaitEvent(_stream_handle(stream), self.ev, 0) != 0:
            raise RuntimeError("hipStreamWaitEvent failed")

    def query(self):
        """True when the event has completed (or was never recorded), False while pending"""
        self.hip.hipEventQuery.argtypes = [ctypes.c_void_p]
        r = self.hip.hipEventQuery(self.ev)
        if r not in (0, 600):  # hipSuccess, hipErrorNotReady
            raise RuntimeError(f"hipEventQuery failed ({r})")
        return r == 0

    def __del__(self):
        try:
            # a registration still pending for this event must not outlive it
            lib().mbls_msm_accumulate_event_drop(self.ev)
            self.hip.hipEventDestroy(self.ev)
        except Exception:
            pass


def scratch_stats():
    """(library scratch hipMallocs, hipFrees, bytes held, pool contexts)"""
    m, f, b = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    c = ctypes.c_int()
    lib().mbls_scratch_stats(ctypes.byref(m), ctypes.byref(f), ctypes.byref(b), ctypes.byref(c))
    return m.value, f.value, b.value, c.value


def release_stream(stream):
    check(lib().mbls_release_stream(_stream_handle(stream)), "mbls_release_stream")


def release_scratch():
    check(lib().mbls_release_scratch(), "mbls_release_scratch")


def sum_jacobian(group, pts_dev, out_dev, stream=None):
    fn = lib().mbls_g1_sum_jacobian if group == "g1" else lib().mbls_g2_sum_jacobian
    check(fn(_p(pts_dev), pts_dev.shape[0], _p(out_dev), _stream_handle(stream)), "sum_jacobian")


def jacobian_to_icicle(group, pts_dev, stream=None):
    fn = lib().mbls_g1_jacobian_to_icicle if group == "g1" else lib().mbls_g2_jacobian_to_icicle
    check(fn(_p(pts_dev), pts_dev.shape[0], _stream_handle(stream)), "jacobian_to_icicle")


def torch_u64(shape_or_array, device="cuda"):
    """uint64 limb storage on the device (int64 dtype: torch is only the allocator)."""
    import torch
    if isinstance(shape_or_array, np.ndarray):
        return torch.from_numpy(shape_or_array.view(np.int64)).to(device)
    return torch.zeros(shape_or_array, dtype=torch.int64, device=device)


def to_numpy_u64(t):
    return t.detach().cpu().numpy().view(np.uint64)


def msm_precompute_strict(on=True):
    """mbls_msm_precompute_strict: precompute_factor > 1 only for tables precompute_bases wrote
    (include/bls12_381_mi355x.h); process-wide"""
    check(lib().mbls_msm_precompute_strict(1 if on else 0), "mbls_msm_precompute_strict")
