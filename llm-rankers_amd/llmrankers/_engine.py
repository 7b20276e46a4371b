"""ctypes binding of librk_engine.so (C ABI: include/rk_engine.h).

north_star asks for a "thin C-ABI cffi layer"; cffi is not installed in this image,
so the same extern "C" surface is bound with the stdlib's ctypes.  There is no fallback: if the shared
library is missing or no gfx950 device is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "librk_engine.so")

RK_F32, RK_F16, RK_BF16 = 0, 1, 2


class RkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rk_engine error {code}: {msg}")
        self.code = code


class RkModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab", "d_model", "n_heads", "d_kv", "d_ff", "n_enc_layers",
                                         "n_dec_layers", "n_buckets", "max_distance", "gated_gelu", "tied_head")] + \
               [("eps", C.c_float)] + [(n, C.c_int32) for n in ("max_tokens", "max_seqs", "max_dec_len")]


class RkLlamaDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab", "hidden", "n_heads", "n_kv_heads", "head_dim", "intermediate", "n_layers",
                                         "tied_head")] + [("eps", C.c_float), ("rope_theta", C.c_float)] + \
               [(n, C.c_int32) for n in ("max_tokens", "max_seqs")]


class RkDebugGemmCall(C.Structure):
    """rk_debug_gemm_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("epi", "family", "M", "N", "K", "lda", "ldw", "ldc")] + \
               [("A", C.c_void_p), ("a_elems", C.c_int64), ("W", C.c_void_p), ("w_elems", C.c_int64),
                ("C", C.c_void_p), ("c_elems", C.c_int64), ("c_off", C.c_int64), ("C_out", C.c_void_p), ("idx_out", C.c_void_p),
                ("band_rows", C.c_int), ("rowscale", C.c_void_p), ("ssq_in", C.c_void_p), ("nb_in", C.c_int), ("factors_kernel", C.c_int),
                ("xraw_out", C.c_void_p), ("ssq_out", C.c_void_p), ("ssq_cap", C.c_int64),
                ("n_split", C.c_int), ("split_stride", C.c_int64), ("batch", C.c_int), ("bsA", C.c_int64), ("bsW", C.c_int64), ("bsC", C.c_int64),
                ("labels", C.c_void_p), ("xlab", C.c_void_p), ("plan_only", C.c_int)] + \
               [(n, C.c_int) for n in ("out_family", "out_variant", "out_m_pp2", "out_ksplit", "out_nb", "out_n_cu")] + \
               [("out_eps", C.c_float), ("out_xs", C.c_float)]


class RkDebugGemmChainCall(C.Structure):
    """rk_debug_gemm_chain_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("epi", "family", "M", "N", "K", "lda", "ldw", "ldc", "n_launch", "accumulate")] + \
               [("A", C.c_void_p), ("a_elems", C.c_int64), ("W", C.c_void_p), ("w_elems", C.c_int64),
                ("C", C.c_void_p), ("c_elems", C.c_int64), ("C_out", C.c_void_p), ("band_rows", C.c_int), ("rowscale", C.c_void_p)] + \
               [(n, C.c_int) for n in ("bg_epi", "bg_family", "bg_M", "bg_N", "bg_K", "bg_variant", "bg_per_fg", "bg_first", "plan_only",
                                       "out_family", "out_variant", "out_m_pp2", "out_ksplit", "out_n_cu",
                                       "bg_out_family", "bg_out_variant", "bg_out_m_pp2", "bg_out_ksplit")]


class RkDebugAttnCall(C.Structure):
    """rk_debug_attn_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("kind", "n_seq", "H", "n_kv", "Ld", "cross", "M", "row0", "d", "P",
                                       "ldq", "ldkv", "ldctx", "k_col", "v_col", "band_rows")] + \
               [("q", C.c_void_p), ("q_rows", C.c_int64), ("kv", C.c_void_p), ("kv_rows", C.c_int64),
                ("seq_off", C.c_void_p), ("row_off", C.c_void_p), ("tree_keys", C.c_void_p), ("tree_pos", C.c_void_p), ("tree_rows", C.c_int),
                ("row_seq", C.c_void_p), ("n_row_seq", C.c_int), ("pos", C.c_void_p), ("bias_lut", C.c_void_p),
                ("cos_t", C.c_void_p), ("sin_t", C.c_void_p), ("max_pos", C.c_int), ("qkv_bias", C.c_void_p),
                ("out", C.c_void_p), ("out_rows", C.c_int64), ("out_all", C.c_void_p), ("cache", C.c_void_p), ("cache_all", C.c_void_p),
                ("plan_only", C.c_int), ("out_kind", C.c_int), ("out_tparam", C.c_int), ("out_grid", C.c_int * 3), ("out_grid2", C.c_int * 3)] + \
               [(n, C.c_int) for n in ("out_lds", "out_staged", "out_mfma", "out_part", "out_R", "out_nch", "out_skip_long",
                                       "out_heads_per_wg", "out_n_cu")] + \
               [("qk_norm", C.c_void_p), ("qk_eps", C.c_float), ("g1", C.c_int), ("live", C.c_void_p)]


class RkDebugXattnChainCall(C.Structure):
    """rk_debug_xattn_chain_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("M", "Ld", "H", "d", "n_seq", "row0", "ldx", "ldo", "band_rows", "fuse_asked")] + \
               [("x", C.c_void_p), ("wq", C.c_void_p), ("wk", C.c_void_p), ("wv", C.c_void_p), ("enc", C.c_void_p), ("enc_rows", C.c_int64),
                ("seq_off", C.c_void_p), ("row_seq", C.c_void_p), ("n_row_seq", C.c_int), ("rowscale", C.c_void_p), ("ssq_in", C.c_void_p),
                ("nb_in", C.c_int), ("ctx", C.c_void_p), ("qk_all", C.c_void_p), ("part_all", C.c_void_p), ("stat_all", C.c_void_p),
                ("xctx_all", C.c_void_p), ("ctx_all", C.c_void_p), ("ws_fill", C.c_uint32), ("plan_only", C.c_int)] + \
               [(n, C.c_int) for n in ("out_fused", "out_block_rows", "out_n_blocks", "out_nch", "out_n_cu")] + \
               [("out_qk_R", C.c_int * 2), ("out_qk_CS", C.c_int * 2), ("out_part_kind", C.c_int * 2), ("out_part_grid", (C.c_int * 3) * 2),
                ("out_fuse_cv", C.c_int * 2), ("out_cv_R", C.c_int * 2), ("out_eps", C.c_float), ("out_xs", C.c_float)]


class RkDebugRowsIn(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_int64), ("off", C.c_int64)]


class RkDebugRowsOut(C.Structure):
    _fields_ = [("interior", C.c_void_p), ("bytes", C.c_int64), ("band", C.c_int64), ("all", C.c_void_p)]


class RkDebugRowsCall(C.Structure):
    """rk_debug_rows_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("op", "kind", "rows", "d", "vocab", "src_rows", "n_out", "nb", "n_pos", "H", "n_kv", "hd", "ld", "P",
                                       "n_slots", "max_pos", "false_id", "true_id", "dec_len", "max_new", "n_steps", "max_admit")] + \
               [("eps", C.c_float), ("xs", C.c_float), ("out_scale", C.c_float), ("in_", RkDebugRowsIn * 4), ("out", RkDebugRowsOut * 8),
                ("plan_only", C.c_int), ("out_grid", C.c_int * 3), ("out_tparam", C.c_int), ("out_variant", C.c_int)]


class RkDebugDraftStepsCall(C.Structure):
    """rk_debug_draft_steps_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("n_slots", "g1", "n_steps", "max_admit", "max_tokens")] + \
               [("script", C.c_void_p), ("script_ints", C.c_int64), ("state", RkDebugRowsOut * 14)]


DRAFT_ARRAYS = ("st", "len", "col", "max_new", "done", "out", "rnext", "rpos", "rlive", "dlen", "nstep", "tabn", "tab", "hist")


class RkDebugGraphStats(C.Structure):
    """rk_debug_graph_stats_t of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("n_keys", "n_ready", "max_keys")] + \
               [(n, C.c_int64) for n in ("eager", "captures", "replays", "failed", "evictions")]


BUFFER_NAMES = ("logits", "amax_val", "amax_idx", "kv_cache", "gen_buf", "lkv", "lpart", "lints")     # RK_DEBUG_BUFFER_NAMES


class RkDebugBuffers(C.Structure):
    """rk_debug_buffers_t of include/rk_engine.h, field for field."""
    _fields_ = [("addr", C.c_uint64 * len(BUFFER_NAMES)), ("cap", C.c_uint64 * len(BUFFER_NAMES))] + \
               [(n, C.c_int) for n in ("amax_gen", "kv_gen", "lkv_gen")]


class RkDebugSampleCall(C.Structure):
    """rk_debug_sample_call of include/rk_engine.h, field for field."""
    _fields_ = [("rows", C.c_int), ("logit_rows", C.c_int), ("V", C.c_int), ("temperature", C.c_float), ("top_k", C.c_int),
                ("top_p", C.c_float), ("logits", C.c_void_p), ("seeds", C.c_void_p), ("index", C.c_void_p),
                ("out_token", C.c_void_p), ("out_kept_k", C.c_void_p), ("out_kept_p", C.c_void_p)]


DEBUG_SENTINEL = 0xCD                    # RK_DEBUG_SENTINEL: the byte the guard bands of rk_debug_gemm_ex are filled with
DEBUG_BAND_ROWS = 256
GEMM_OUT_DTYPE = {0: np.float16, 1: np.float32, 2: np.float16, 3: np.float16, 4: np.float32, 5: np.float16, 6: np.float32, 7: np.float32}

# name -> (restype, argtypes); this table is also what tests check against include/rk_engine.h
_P = C.POINTER
_i32p, _f32p = _P(C.c_int32), _P(C.c_float)
ABI = {
    "rk_engine_create": (C.c_int, [_P(RkModelDesc), C.c_int, _P(C.c_void_p)]),
    "rk_engine_destroy": (None, [C.c_void_p]),
    "rk_last_error": (C.c_char_p, [C.c_void_p]),
    "rk_engine_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, _P(C.c_int64), C.c_int]),
    "rk_engine_finalize": (C.c_int, [C.c_void_p]),
    "rk_t5_score": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _i32p, C.c_int, _f32p]),
    "rk_t5_compare": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _i32p]),
    "rk_t5_qlm": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _f32p]),
    "rk_t5_qlm_many": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, _i32p, _f32p]),
    "rk_t5_greedy": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p]),
    "rk_t5_greedy2": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _i32p]),
    "rk_t5_generate": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p]),
    "rk_t5_stage": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int]),
    "rk_t5_score_staged": (C.c_int, [C.c_void_p, _i32p, C.c_int, _i32p, C.c_int]),
    "rk_engine_sync": (C.c_int, [C.c_void_p]),
    "rk_engine_num_slots": (C.c_int, []),
    "rk_t5_stage_slot": (C.c_int, [C.c_void_p, C.c_int, _i32p, _i32p, C.c_int]),
    "rk_t5_score_slot": (C.c_int, [C.c_void_p, C.c_int, _i32p, C.c_int, _i32p, C.c_int]),
    "rk_t5_compare_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rk_t5_read_scores_slot": (C.c_int, [C.c_void_p, C.c_int, _f32p, C.c_int]),
    "rk_t5_read_scores": (C.c_int, [C.c_void_p, _f32p, C.c_int]),
    "rk_t5_scores_device_ptr": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "rk_llama_create": (C.c_int, [_P(RkLlamaDesc), C.c_int, _P(C.c_void_p)]),
    "rk_llama_set_rope_scaling": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]),
    "rk_llama_set_qkv_bias": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_llama_set_qk_norm": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_llama_set_sliding_window": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_llama_set_weight_fp8": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_llama_greedy1": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p]),
    "rk_llama_last_logits": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _f32p]),
    "rk_llama_generate": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _i32p, _i32p]),
    "rk_llama_set_sampling": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_float]),
    "rk_llama_generate_sampled": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, _i32p, _i32p,
                                            _P(C.c_uint64)]),
    "rk_llama_session_admit_sampled": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _i32p, C.c_int, _P(C.c_uint64)]),
    "rk_debug_sample": (C.c_int, [C.c_void_p, _P(RkDebugSampleCall)]),
    "rk_llama_session_open": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int]),
    "rk_llama_session_admit": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _i32p, C.c_int]),
    "rk_llama_session_run": (C.c_int, [C.c_void_p, C.c_int, _i32p, _i32p, _i32p]),
    "rk_llama_session_read": (C.c_int, [C.c_void_p, C.c_int, _i32p, C.c_int, _i32p]),
    "rk_llama_session_close": (C.c_int, [C.c_void_p]),
    "rk_llama_session_open_draft": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rk_llama_session_stats": (C.c_int, [C.c_void_p, _P(C.c_int64), _P(C.c_int64), _i32p, _i32p]),
    "rk_debug_session_drafts": (C.c_int, [C.c_void_p, C.c_int, _i32p, C.c_int]),
    "rk_comm_unique_id": (C.c_int, [_P(C.c_uint8), C.c_int]),
    "rk_comm_init": (C.c_int, [C.c_void_p, _P(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int]),
    "rk_comm_world": (C.c_int, [C.c_void_p, _i32p, _i32p]),
    "rk_comm_capacity": (C.c_int, [C.c_void_p]),
    "rk_comm_library_info": (C.c_int, [C.c_char_p, C.c_int]),
    "rk_comm_append_host": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int]),
    "rk_comm_all_gather_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rk_comm_read_gathered_slot": (C.c_int, [C.c_void_p, C.c_int, _f32p, C.c_int]),
    "rk_comm_append_scores_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rk_comm_all_gather_appended": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_comm_read_appended": (C.c_int, [C.c_void_p, _f32p, C.c_int]),
    "rk_comm_destroy": (C.c_int, [C.c_void_p]),
    "rk_timer_begin": (C.c_int, [C.c_void_p]),
    "rk_timer_end": (C.c_int, [C.c_void_p, _f32p]),
    "rk_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_profile_reset": (C.c_int, [C.c_void_p]),
    "rk_profile_num_classes": (C.c_int, []),
    "rk_profile_class_name": (C.c_char_p, [C.c_int]),
    "rk_profile_get": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_double), _P(C.c_int64), _P(C.c_double), _P(C.c_double)]),
    "rk_engine_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "rk_abi_version": (C.c_int, []),
    "rk_rel_bucket": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "rk_debug_gemm": (C.c_int, [C.c_void_p, _P(C.c_uint16), _P(C.c_uint16), _f32p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rk_debug_gemm_ex": (C.c_int, [C.c_void_p, _P(RkDebugGemmCall)]),
    "rk_debug_quant_fp8": (C.c_int, [C.c_void_p, _P(C.c_uint16), C.c_int, C.c_int, C.c_int, _P(C.c_uint8), _P(C.c_int8), _P(C.c_uint16)]),
    "rk_debug_gemm_fp8": (C.c_int, [C.c_void_p, _P(RkDebugGemmCall)]),
    "rk_debug_gemm_chain": (C.c_int, [C.c_void_p, _P(RkDebugGemmChainCall)]),
    "rk_debug_attn": (C.c_int, [C.c_void_p, _P(RkDebugAttnCall)]),
    "rk_debug_xattn_chain": (C.c_int, [C.c_void_p, _P(RkDebugXattnChainCall)]),
    "rk_debug_rows": (C.c_int, [C.c_void_p, _P(RkDebugRowsCall)]),
    "rk_debug_draft_steps": (C.c_int, [C.c_void_p, _P(RkDebugDraftStepsCall)]),
    "rk_debug_gemm_bench": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "rk_debug_read": (C.c_int64, [C.c_void_p, C.c_char_p, _f32p, C.c_int64]),
    "rk_debug_graph_stats": (C.c_int, [C.c_void_p, _P(RkDebugGraphStats)]),
    "rk_debug_buffers": (C.c_int, [C.c_void_p, _P(RkDebugBuffers)]),
}

_lib = None


def load_library(path: Optional[str] = None, make_default: bool = False):
    """dlopen librk_engine.so and attach prototypes. Raises if the in-tree build is missing (no fallback).
    The product always loads the in-tree library (LIB_PATH).  `path` + make_default=True is for tools/ only: separately compiled
    A/B or measurement builds (tools/_lib.py); no environment variable redirects the product's library."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  If torch gets imported AFTER this library (e.g. via
    # transformers' tokenizer), the process would hold two HIP runtimes; importing torch first lets the loader
    # resolve our DT_NEEDED libamdhip64.so.7 to the copy already mapped.  Plumbing only — nothing here uses torch.
    if os.environ.get("RK_IMPORT_TORCH_FIRST", "1") == "1":
        import sys
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} not found: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU/PyTorch fallback for the hot path.")
    lib = C.CDLL(p)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)     # AttributeError here = the .so does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    if path is None or make_default:
        _lib = lib
    return lib


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _seeds(seeds, n: int) -> np.ndarray:
    """n 64-bit seeds as the engine takes them (Python ints are reduced mod 2^64)."""
    if len(seeds) != n:
        raise ValueError(f"{n} prompts but {len(seeds)} seeds")
    return np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)


def pack_ragged(seqs: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """list of token-id sequences -> (tokens[T] int32, seq_offsets[B+1] int32): the engine's input boundary."""
    lens = [len(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    tok = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if seqs else np.zeros(0, np.int32)
    return np.ascontiguousarray(tok, dtype=np.int32), off


class RkEngine:
    """One engine = one MI355X.  Thin object wrapper; all compute happens in the HIP library."""

    def __init__(self, dims, device: int = 0, max_tokens: int = 16384, max_seqs: int = 128, max_dec_len: int = 136):
        self.lib = load_library()
        self.dims = dims
        self.desc = RkModelDesc(vocab=dims.vocab, d_model=dims.d_model, n_heads=dims.n_heads, d_kv=dims.d_kv,
                                d_ff=dims.d_ff, n_enc_layers=dims.n_enc, n_dec_layers=dims.n_dec,
                                n_buckets=dims.n_buckets, max_distance=dims.max_distance,
                                gated_gelu=int(dims.gated), tied_head=int(dims.tied_head), eps=dims.eps,
                                max_tokens=max_tokens, max_seqs=max_seqs, max_dec_len=max_dec_len)
        h = C.c_void_p()
        rc = self.lib.rk_engine_create(C.byref(self.desc), device, C.byref(h))
        if rc != 0:
            raise RkError(rc, (self.lib.rk_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self.comm_rank, self.comm_world = 0, 1

    # -- plumbing ------------------------------------------------------------------------------------
    def _chk(self, rc: int):
        if rc != 0:
            raise RkError(rc, (self.lib.rk_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rk_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -------------------------------------------------------------------------------------
    def load_tensor(self, name: str, arr: np.ndarray):
        if arr.dtype == np.float16:
            dt = RK_F16
        elif arr.dtype == np.float32:
            dt = RK_F32
        elif arr.dtype == np.uint16:      # raw bf16 bits (safetensors bf16 viewed as uint16)
            dt = RK_BF16
        else:
            arr, dt = arr.astype(np.float32), RK_F32
        arr = np.ascontiguousarray(arr)
        shape = (C.c_int64 * arr.ndim)(*arr.shape)
        self._chk(self.lib.rk_engine_load_tensor(self.h, name.encode(), arr.ctypes.data_as(C.c_void_p), dt, shape, arr.ndim))

    def load_state(self, tensors: Iterable[Tuple[str, np.ndarray]]):
        for name, arr in tensors:
            self.load_tensor(name, arr)
        self._chk(self.lib.rk_engine_finalize(self.h))
        return self

    # -- the three call shapes of the hot path ----------------------------------------------------------
    def score(self, seqs: Sequence[Sequence[int]], dec_prefix: Sequence[int], out_ids: Sequence[int]) -> np.ndarray:
        tok, off = pack_ragged(seqs)
        dp, oi = _i32(dec_prefix), _i32(out_ids)
        out = np.empty((len(seqs), len(oi)), dtype=np.float32)
        self._chk(self.lib.rk_t5_score(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                       dp.ctypes.data_as(_i32p), len(dp), oi.ctypes.data_as(_i32p), len(oi),
                                       out.ctypes.data_as(_f32p)))
        return out

    def compare_pairs(self, seqs: Sequence[Sequence[int]], dec_start: int, false_id: int, true_id: int):
        """The duoT5 compare (rk_t5_compare): seqs = 2n sequences, pair p = (seqs[2p], seqs[2p + 1]) = the A/B and the B/A prompt.
        -> (logits [2n, 2] = (false, true), p_true [2n], first_wins [n] bool), softmax and verdict taken on the device."""
        if len(seqs) % 2:
            raise ValueError(f"a compare needs pairs of sequences (got {len(seqs)})")
        tok, off = pack_ragged(seqs)
        n = len(seqs) // 2
        logits, p_true, wins = np.empty((2 * n, 2), np.float32), np.empty(2 * n, np.float32), np.empty(n, np.int32)
        self._chk(self.lib.rk_t5_compare(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), n, int(dec_start),
                                         int(false_id), int(true_id), logits.ctypes.data_as(_f32p), p_true.ctypes.data_as(_f32p),
                                         wins.ctypes.data_as(_i32p)))
        return logits, p_true, wins != 0

    def qlm(self, seqs: Sequence[Sequence[int]], labels: Sequence[int]) -> np.ndarray:
        tok, off = pack_ragged(seqs)
        lab = _i32(labels)
        out = np.empty(len(seqs), dtype=np.float32)
        self._chk(self.lib.rk_t5_qlm(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                     lab.ctypes.data_as(_i32p), len(lab), out.ctypes.data_as(_f32p)))
        return out

    def qlm_many(self, seqs: Sequence[Sequence[int]], labels_per_seq: Sequence[Sequence[int]]) -> np.ndarray:
        """qlm scores of sequences that each score their OWN label sequence, in one engine call (rk_t5_qlm_many): element b is
        bit for bit qlm([seqs[b]], labels_per_seq[b])[0] in a batch that stays off the few-row family."""
        if len(labels_per_seq) != len(seqs):
            raise ValueError(f"{len(seqs)} sequences but {len(labels_per_seq)} label sequences")
        tok, off = pack_ragged(seqs)
        lab, loff = pack_ragged(labels_per_seq)
        out = np.empty(len(seqs), dtype=np.float32)
        self._chk(self.lib.rk_t5_qlm_many(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                          lab.ctypes.data_as(_i32p), loff.ctypes.data_as(_i32p), out.ctypes.data_as(_f32p)))
        return out

    def greedy(self, seqs: Sequence[Sequence[int]], dec_prefix: Sequence[int], max_new: int, eos_id: int = 1,
               pad_id: int = 0, candidates: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, int]:
        """`candidates` (max_new == 2 only): token ids the first new token is expected to be among - same result, one
        decoder pass instead of two (rk_t5_greedy2)."""
        tok, off = pack_ragged(seqs)
        dp = _i32(dec_prefix)
        out = np.empty((len(seqs), max_new), dtype=np.int32)
        steps = C.c_int32(0)
        if candidates is not None and len(candidates) and max_new == 2:
            cd = _i32(candidates)
            self._chk(self.lib.rk_t5_greedy2(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                             dp.ctypes.data_as(_i32p), len(dp), cd.ctypes.data_as(_i32p), len(cd), eos_id, pad_id,
                                             out.ctypes.data_as(_i32p), C.byref(steps)))
            return out, int(steps.value)
        self._chk(self.lib.rk_t5_greedy(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                        dp.ctypes.data_as(_i32p), len(dp), max_new, eos_id, pad_id,
                                        out.ctypes.data_as(_i32p), C.byref(steps)))
        return out, int(steps.value)

    def generate(self, seqs: Sequence[Sequence[int]], dec_prefix: Sequence[int], max_new: int, eos_id: int = 1,
                 pad_id: int = 0) -> Tuple[np.ndarray, int]:
        """`greedy`'s result (tokens [B, max_new], decoder steps) from the KV-cached incremental decoder (rk_t5_generate): one
        decoder row per sequence and step instead of the whole prefix - for long continuations (listwise permutations)."""
        tok, off = pack_ragged(seqs)
        dp = _i32(dec_prefix)
        out = np.empty((len(seqs), max_new), dtype=np.int32)
        steps = C.c_int32(0)
        self._chk(self.lib.rk_t5_generate(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                          dp.ctypes.data_as(_i32p), len(dp), max_new, eos_id, pad_id,
                                          out.ctypes.data_as(_i32p), C.byref(steps)))
        return out, int(steps.value)

    # -- staged / async form (bench, multi-GPU) --------------------------------------------------------
    @property
    def num_slots(self) -> int:
        return int(self.lib.rk_engine_num_slots())

    def stage(self, seqs: Sequence[Sequence[int]], slot: int = 0):
        tok, off = pack_ragged(seqs)
        self._chk(self.lib.rk_t5_stage_slot(self.h, slot, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs)))
        self._slot_shape = getattr(self, "_slot_shape", {})
        self._slot_shape[slot] = [len(seqs), 0]

    def score_staged(self, dec_prefix: Sequence[int], out_ids: Sequence[int], slot: int = 0):
        """Enqueue encoder (encoder stream) + decoder/head (decoder stream) for the slot's batch; returns at once."""
        dp, oi = _i32(dec_prefix), _i32(out_ids)
        self._slot_shape[slot][1] = len(oi)
        self._chk(self.lib.rk_t5_score_slot(self.h, slot, dp.ctypes.data_as(_i32p), len(dp), oi.ctypes.data_as(_i32p), len(oi)))

    def compare_staged(self, dec_start: int, false_id: int, true_id: int, slot: int = 0):
        """score_staged's twin for the duoT5 compare (rk_t5_compare_slot) over the slot's staged pairs; `read_scores` then gives
        compare_pairs' triple."""
        self._slot_shape[slot][1] = None
        self._chk(self.lib.rk_t5_compare_slot(self.h, slot, int(dec_start), int(false_id), int(true_id)))

    def sync(self):
        self._chk(self.lib.rk_engine_sync(self.h))

    def read_scores(self, slot: int = 0):
        n, k = self._slot_shape[slot]
        if k is None:                    # a compare: logits [n, 2], P(true) [n], verdicts [n / 2] in one buffer of 3.5 n floats
            out = np.empty(3 * n + n // 2, dtype=np.float32)
            self._chk(self.lib.rk_t5_read_scores_slot(self.h, slot, out.ctypes.data_as(_f32p), out.size))
            return out[:2 * n].reshape(n, 2).copy(), out[2 * n:3 * n].copy(), out[3 * n:] != 0
        out = np.empty((n, k), dtype=np.float32)
        self._chk(self.lib.rk_t5_read_scores_slot(self.h, slot, out.ctypes.data_as(_f32p), out.size))
        return out

    def scores_device_ptr(self) -> int:
        p = C.c_void_p()
        self._chk(self.lib.rk_t5_scores_device_ptr(self.h, C.byref(p)))
        return int(p.value)

    # -- multi-GPU score collection (RCCL inside the engine) -----------------------------------------------
    COMM_ID_BYTES = 128

    def comm_unique_id(self) -> bytes:
        """rank 0: the 128-byte RCCL id every rank needs for comm_init (ship it with any host-side channel)."""
        buf = (C.c_uint8 * self.COMM_ID_BYTES)()
        rc = self.lib.rk_comm_unique_id(buf, self.COMM_ID_BYTES)
        if rc != 0:
            raise RkError(rc, (self.lib.rk_last_error(None) or b"").decode())
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int, max_floats_per_rank: int):
        """Collective over all ranks (one engine = one process = one GPU)."""
        buf = (C.c_uint8 * self.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._chk(self.lib.rk_comm_init(self.h, buf, self.COMM_ID_BYTES, rank, world, max_floats_per_rank))
        self.comm_rank, self.comm_world = rank, world
        self.comm_capacity = int(self.lib.rk_comm_capacity(self.h))   # what every rank checks before it enters a gather

    def comm_library_info(self) -> str:
        """'<path of the RCCL library this process bound>|<ncclGetVersion code>' (the torch wheel bundles its own librccl;
        which one served the run belongs in the logs)."""
        buf = C.create_string_buffer(1024)
        n = self.lib.rk_comm_library_info(buf, 1024)
        if n < 0:
            raise RkError(n, (self.lib.rk_last_error(None) or b"").decode())
        return buf.value.decode()

    def comm_append_host(self, values, offset: int):
        """Put host floats at `offset` of the engine's send buffer (side data that travels with the scores in the one gather)."""
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        self._chk(self.lib.rk_comm_append_host(self.h, v.ctypes.data_as(_f32p), v.size, offset))

    def comm_all_gather(self, n_floats: int, slot: int = 0):
        """Enqueue ONE RCCL all_gather of the slot's device score buffer behind the work that fills it (no sync)."""
        self._chk(self.lib.rk_comm_all_gather_slot(self.h, slot, n_floats))
        self._gather_n = getattr(self, "_gather_n", {})
        self._gather_n[slot] = n_floats

    def comm_read_gathered(self, slot: int = 0) -> np.ndarray:
        """[world, n_floats] float32 of the slot's last gather (waits for it)."""
        n = self._gather_n[slot]
        out = np.empty((self.comm_world, n), dtype=np.float32)
        self._chk(self.lib.rk_comm_read_gathered_slot(self.h, slot, out.ctypes.data_as(_f32p), out.size))
        return out

    def comm_append(self, n_floats: int, offset: int, slot: int = 0):
        """Copy the slot's last n_floats scores to `offset` of the engine's send buffer (device to device, no sync)."""
        self._chk(self.lib.rk_comm_append_scores_slot(self.h, slot, n_floats, offset))

    def comm_all_gather_appended(self, n_floats: int) -> np.ndarray:
        """ONE RCCL all_gather of the first n_floats of the send buffer -> [world, n_floats] float32 (waits for it)."""
        self._chk(self.lib.rk_comm_all_gather_appended(self.h, n_floats))
        out = np.empty((self.comm_world, n_floats), dtype=np.float32)
        self._chk(self.lib.rk_comm_read_appended(self.h, out.ctypes.data_as(_f32p), out.size))
        return out

    def comm_destroy(self):
        self._chk(self.lib.rk_comm_destroy(self.h))
        self.comm_rank, self.comm_world, self.comm_capacity = 0, 1, 0

    # -- measurement -------------------------------------------------------------------------------------
    def timer_begin(self):
        self._chk(self.lib.rk_timer_begin(self.h))

    def timer_end(self) -> float:
        ms = C.c_float(0)
        self._chk(self.lib.rk_timer_end(self.h, C.byref(ms)))
        return float(ms.value)

    def profile(self, on: bool):
        self._chk(self.lib.rk_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._chk(self.lib.rk_profile_reset(self.h))

    def profile_report(self) -> dict:
        rep = {}
        for c in range(self.lib.rk_profile_num_classes()):
            ms, n, fl, by = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
            self._chk(self.lib.rk_profile_get(self.h, c, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
            rep[self.lib.rk_profile_class_name(c).decode()] = {"ms": ms.value, "launches": n.value, "flops": fl.value,
                                                              "bytes": by.value}
        return rep

    def set_option(self, key: str, value: int):
        self._chk(self.lib.rk_engine_set_option(self.h, key.encode(), int(value)))

    # -- debug ---------------------------------------------------------------------------------------------
    def debug_gemm(self, a16: np.ndarray, w16: np.ndarray, use_glds=True) -> np.ndarray:
        a16 = np.ascontiguousarray(a16, dtype=np.float16)
        w16 = np.ascontiguousarray(w16, dtype=np.float16)
        m, k = a16.shape
        n = w16.shape[0]
        out = np.empty((m, n), dtype=np.float32)
        self._chk(self.lib.rk_debug_gemm(self.h, a16.view(np.uint16).ctypes.data_as(_P(C.c_uint16)),
                                         w16.view(np.uint16).ctypes.data_as(_P(C.c_uint16)),
                                         out.ctypes.data_as(_f32p), m, n, k, int(use_glds)))
        return out

    def gemm_bench(self, m: int, n: int, k: int, epi: int = 0, iters: int = 20) -> float:
        """average ms per launch of the engine GEMM at (m, n, k)"""
        ms = C.c_float(0)
        self._chk(self.lib.rk_debug_gemm_bench(self.h, m, n, k, epi, iters, C.byref(ms)))
        return float(ms.value)

    def debug_gemm_ex(self, epi: int, family: int, a16: np.ndarray, w16: np.ndarray, M: int, N: int, K: int, *, lda=None, ldw=None,
                      ldc=None, c_in: Optional[np.ndarray] = None, c_off=0, rowscale=None, ssq_in=None, factors_kernel=False,
                      producer=False, n_split=0, split_stride=0, batch=1, bsA=0, bsW=0, bsC=0, labels=None, plan_only=False,
                      entry: str = "rk_debug_gemm_ex") -> dict:
        """One call of the engine's GEMM through rk_debug_gemm_ex (include/rk_engine.h; entry: rk_debug_gemm_fp8's name for its form).  a16 / w16: flat or 2-D fp16 arrays holding
        everything the call addresses; c_in: the flat INTERIOR of the output in the output type (epi 7: two floats per element),
        default = all sentinel bytes.  Returns the plan fields and the WHOLE device allocations after the call, bands included:
        "C" (flat, band | interior | band; "band" = elements per band), "idx", "xraw" [(2 band_rows + M), N], "ssq"
        [(2 band_rows + M), nb], "xlab"."""
        a16 = np.ascontiguousarray(a16, dtype=np.float16).reshape(-1)
        w16 = np.ascontiguousarray(w16, dtype=np.float16).reshape(-1)
        gated, blocks = epi in (2, 5), epi in (6, 7)
        width = -(-N // 32) if blocks else (n_split if n_split else (N // 2 if gated else N))
        lda, ldw, ldc = lda or K, ldw or K, ldc or width
        dt, per = GEMM_OUT_DTYPE[epi], (2 if epi == 7 else 1)
        if c_in is None:
            nsb = -(-N // n_split) if n_split else 1
            c_elems = c_off + (batch - 1) * bsC + (nsb - 1) * split_stride + M * ldc
            c_in = np.frombuffer(bytes([DEBUG_SENTINEL]) * (c_elems * per * np.dtype(dt).itemsize), dtype=dt).copy()
        c_in = np.ascontiguousarray(c_in, dtype=dt).reshape(-1)
        c_elems = c_in.size // per
        band = DEBUG_BAND_ROWS * ldc
        q = RkDebugGemmCall()
        q.epi, q.family, q.M, q.N, q.K, q.lda, q.ldw, q.ldc = epi, family, M, N, K, lda, ldw, ldc
        q.A, q.a_elems, q.W, q.w_elems = a16.ctypes.data, a16.size, w16.ctypes.data, w16.size
        q.C, q.c_elems, q.c_off, q.band_rows = c_in.ctypes.data, c_elems, c_off, DEBUG_BAND_ROWS
        c_out = np.zeros((2 * band + c_elems) * per, dtype=dt)
        q.C_out = c_out.ctypes.data
        keep = [a16, w16, c_in, c_out]
        idx = xraw = ssq = xlab = None
        if epi == 6:
            idx = np.zeros(2 * band + c_elems, dtype=np.int32)
            q.idx_out = idx.ctypes.data
        if rowscale is not None:
            rowscale = np.ascontiguousarray(rowscale, dtype=np.float32)
            assert rowscale.size == M
            q.rowscale = rowscale.ctypes.data
        if ssq_in is not None:
            ssq_in = np.ascontiguousarray(ssq_in, dtype=np.float32)
            assert ssq_in.ndim == 2 and ssq_in.shape[0] == M
            q.ssq_in, q.nb_in, q.factors_kernel = ssq_in.ctypes.data, ssq_in.shape[1], int(factors_kernel)
        rows_all = 2 * DEBUG_BAND_ROWS + M
        if producer:
            xraw = np.zeros((rows_all, N), dtype=np.float16)
            ssq = np.zeros(rows_all * (-(-N // 4) + 1), dtype=np.float32)       # room for any family's block count
            q.xraw_out, q.ssq_out, q.ssq_cap = xraw.ctypes.data, ssq.ctypes.data, ssq.size
        q.n_split, q.split_stride, q.batch, q.bsA, q.bsW, q.bsC = n_split, split_stride, batch, bsA, bsW, bsC
        if epi == 7:
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            assert labels.size == M
            xlab = np.frombuffer(bytes([DEBUG_SENTINEL]) * (4 * M), dtype=np.float32).copy()
            q.labels, q.xlab = labels.ctypes.data, xlab.ctypes.data
        q.plan_only = int(plan_only)
        self._chk(getattr(self.lib, entry)(self.h, C.byref(q)))
        del keep
        out = {k[4:]: getattr(q, k) for k, _ in RkDebugGemmCall._fields_ if k.startswith("out_")}
        if plan_only:
            return out
        out.update(C=c_out, band=band, idx=idx, xlab=xlab, ldc=ldc, c_elems=c_elems)
        if producer:
            out.update(xraw=xraw, ssq=ssq[:rows_all * q.out_nb].reshape(rows_all, q.out_nb))
        return out

    def debug_gemm_fp8(self, epi: int, a16: np.ndarray, w16: np.ndarray, M: int, N: int, K: int, **kw) -> dict:
        """debug_gemm_ex with family = 1 on FP8 step weights (rk_debug_gemm_fp8): w16 goes through the engine's quantiser and the FP8
        weight-streaming kernel forms the product from the bytes.  Same keywords, same result layout."""
        return self.debug_gemm_ex(epi, 1, a16, w16, M, N, K, entry="rk_debug_gemm_fp8", **kw)

    def debug_quant_fp8(self, w16: np.ndarray, K: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The engine's FP8 quantiser on a host matrix (rk_debug_quant_fp8; the format: include/rk_engine.h at rk_llama_set_weight_fp8).
        w16: fp16 [N, ldw]; K (default ldw): the columns that count.  Returns (e4m3fn bytes [N, K] uint8 row-major, exponents
        [N, ceil(K / 128)] int8, the dequantised fp16 matrix [N, K])."""
        w16 = np.ascontiguousarray(w16, dtype=np.float16)
        N, ld = w16.shape
        K = ld if K is None else int(K)
        q = np.zeros((N, K), dtype=np.uint8)
        ex = np.zeros((N, -(-K // 128)), dtype=np.int8)
        deq = np.zeros((N, K), dtype=np.float16)
        self._chk(self.lib.rk_debug_quant_fp8(self.h, w16.ctypes.data_as(_P(C.c_uint16)), N, K, ld, q.ctypes.data_as(_P(C.c_uint8)),
                                              ex.ctypes.data_as(_P(C.c_int8)), deq.ctypes.data_as(_P(C.c_uint16))))
        return q, ex, deq

    def debug_gemm_chain(self, epi: int, a16: np.ndarray, w16: np.ndarray, M: int, N: int, K: int, *, family=0, ldc=None,
                         c_in: Optional[np.ndarray] = None, accumulate=False, rowscale=None, bg: Optional[dict] = None, bg_per_fg=0,
                         bg_first=True, n_launch=None, plan_only=False, c_out: Optional[np.ndarray] = None) -> dict:
        """n_launch back-to-back launches of one GEMM call with new data per launch through rk_debug_gemm_chain (include/rk_engine.h).
        a16: fp16 [n_launch, M, K] (launch i's A); w16: fp16 [N, K], shared; rowscale: [n_launch, M] or None; c_in: [n_out, M * ldc]
        interiors in the output type, n_out = 1 with accumulate (epi 1) else n_launch, default all sentinel bytes; bg: dict(epi, family,
        M, N, K, variant) of the background call, bg_per_fg launches of it per foreground launch on the decoder stream.  c_out: the host
        array the allocations are read back into (default: a new one, sentinel-filled).  Returns the plan fields ("bg_family", ... for
        the background's) and "C" [n_out, band + M * ldc + band]: the whole device allocations after the last launch."""
        a16 = np.ascontiguousarray(a16, dtype=np.float16)
        w16 = np.ascontiguousarray(w16, dtype=np.float16).reshape(-1)
        nl = a16.shape[0] if n_launch is None else int(n_launch)
        a_elems = a16.size // max(1, a16.shape[0])
        width = N // 2 if epi in (2, 5) else N
        ldc = ldc or width
        dt = GEMM_OUT_DTYPE[epi]
        n_out = 1 if accumulate else max(1, a16.shape[0])
        c_elems, band = M * ldc, DEBUG_BAND_ROWS * ldc
        q = RkDebugGemmChainCall()
        if not plan_only:
            if c_in is None:
                c_in = np.frombuffer(bytes([DEBUG_SENTINEL]) * (n_out * c_elems * np.dtype(dt).itemsize), dtype=dt).copy()
            c_in = np.ascontiguousarray(c_in, dtype=dt).reshape(-1)
            assert c_in.size == n_out * c_elems
            if c_out is None:
                c_out = np.frombuffer(bytes([DEBUG_SENTINEL]) * (n_out * (2 * band + c_elems) * np.dtype(dt).itemsize), dtype=dt).copy()
            assert c_out.dtype == dt and c_out.size == n_out * (2 * band + c_elems) and c_out.flags["C_CONTIGUOUS"]
            q.C, q.C_out = c_in.ctypes.data, c_out.ctypes.data
        q.epi, q.family, q.M, q.N, q.K, q.lda, q.ldw, q.ldc, q.n_launch, q.accumulate = epi, family, M, N, K, K, K, ldc, nl, int(accumulate)
        q.A, q.a_elems, q.W, q.w_elems = a16.ctypes.data, a_elems, w16.ctypes.data, w16.size
        q.c_elems, q.band_rows = c_elems, DEBUG_BAND_ROWS
        if rowscale is not None:
            rowscale = np.ascontiguousarray(rowscale, dtype=np.float32)
            assert rowscale.shape == (a16.shape[0], M)
            q.rowscale = rowscale.ctypes.data
        if bg is not None:
            q.bg_epi, q.bg_family, q.bg_M, q.bg_N, q.bg_K, q.bg_variant = bg["epi"], bg["family"], bg["M"], bg["N"], bg["K"], bg.get("variant", 0)
            q.bg_per_fg, q.bg_first = int(bg_per_fg), int(bg_first)
        q.plan_only = int(plan_only)
        self._chk(self.lib.rk_debug_gemm_chain(self.h, C.byref(q)))
        out = {k[4:]: getattr(q, k) for k, _ in RkDebugGemmChainCall._fields_ if k.startswith("out_")}
        out.update({"bg_" + k[7:]: getattr(q, k) for k, _ in RkDebugGemmChainCall._fields_ if k.startswith("bg_out_")})
        if not plan_only:
            out.update(C=c_out.reshape(n_out, 2 * band + c_elems), band=band, ldc=ldc)
        return out

    def debug_attn(self, kind: int, *, n_seq: int, H: int, q=None, out=None, kv=None, band_rows=8, n_kv=0, Ld=0, cross=False, M=0, row0=0,
                   d=0, P=0, ldq=0, ldkv=0, ldctx=0, k_col=0, v_col=0, seq_off=None, row_off=None, tree_keys=None, tree_pos=None,
                   row_seq=None, pos=None, bias_lut=None, cos=None, sin=None, qkv_bias=None, cache=None, plan_only=False,
                   qk_norm=None, qk_eps=0.0, g1=0, live=None) -> dict:
        """One attention call through rk_debug_attn (include/rk_engine.h).  q / kv: 2-D fp16 [band_rows + rows + band_rows, ld], the
        WHOLE allocation with the caller's bands; out: 2-D fp16 [rows, ldctx], the pre-filled interior; cache (kind 5): flat fp16, K then
        V (kind 6, the T5 cached step: [n_seq][P][k | v] of 64 H each, bands of band_rows * 64 elements, pos one value).  Returns the plan fields and, unless plan_only, "out" [band_rows + rows + band_rows, ldctx] and "cache" (flat, with bands
        of band_rows * hd elements, hd = a Llama engine's head width): the whole device allocations after the call."""
        hd = int(getattr(self.desc, "head_dim", 128))   # the Llama kinds' head width (64 or 128); the T5 kinds have no such operand
        c = RkDebugAttnCall()
        c.kind, c.n_seq, c.H, c.n_kv, c.Ld, c.cross, c.M, c.row0, c.d, c.P = kind, n_seq, H, n_kv, Ld, int(cross), M, row0, d, P
        c.ldq, c.ldkv, c.ldctx, c.k_col, c.v_col, c.band_rows, c.plan_only = ldq, ldkv, ldctx, k_col, v_col, band_rows, int(plan_only)
        keep = []

        def put(field, a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            setattr(c, field, a.ctypes.data)
            return a

        if q is not None:
            q = put("q", q, np.float16)
            assert q.ndim == 2 and q.shape[1] == ldq and q.shape[0] >= 2 * band_rows
            c.q_rows = q.shape[0] - 2 * band_rows
        if kv is not None:
            kv = put("kv", kv, np.float16)
            assert kv.ndim == 2 and kv.shape[1] == ldkv and kv.shape[0] >= 2 * band_rows
            c.kv_rows = kv.shape[0] - 2 * band_rows
        for name, a in (("seq_off", seq_off), ("row_off", row_off), ("tree_keys", tree_keys), ("tree_pos", tree_pos), ("row_seq", row_seq), ("pos", pos)):
            a = put(name, a, np.int32)
            if a is not None:
                assert a.size >= {"seq_off": n_seq + 1, "row_off": n_seq + 1, "pos": 1 if kind == 6 else n_seq}.get(name, 0)
                if name == "tree_pos":
                    c.tree_rows = a.size
                    assert tree_keys is not None and np.asarray(tree_keys).size == a.size * Ld
                if name == "row_seq":
                    c.n_row_seq = a.size
        if bias_lut is not None:
            assert put("bias_lut", bias_lut, np.float32).shape == (H, 257)
        if cos is not None:
            cos, sin = put("cos_t", cos, np.float32), put("sin_t", sin, np.float32)
            assert cos.ndim == 2 and cos.shape[1] == hd // 2 and sin.shape == cos.shape
            c.max_pos = cos.shape[0]
        if qkv_bias is not None:
            assert put("qkv_bias", qkv_bias, np.float32).size == (H + 2 * n_kv) * hd
        if qk_norm is not None:                              # kind 5: Qwen3's q | k head-norm weights, the step's entry with the norm
            assert put("qk_norm", qk_norm, np.float32).size == 2 * hd
            c.qk_eps = float(qk_eps)
        c.g1 = int(g1)                                       # kind 5: a drafting step, g1 step rows per cache row (0 / 1: the plain call)
        if live is not None:
            assert put("live", live, np.int32).size == n_seq
        out_all = cache_all = None
        if out is not None:
            out = put("out", out, np.float16)
            assert out.ndim == 2 and out.shape[1] == ldctx
            c.out_rows = out.shape[0]
            out_all = put("out_all", np.zeros((out.shape[0] + 2 * band_rows, ldctx)), np.float16)
        if cache is not None:
            cache = put("cache", cache, np.float16).reshape(-1)
            if kind == 6:                                   # the T5 cached step: [n_seq][P][k | v] of 64 H each, bands of band_rows x 64
                hd = 64
                assert cache.size == n_seq * P * 2 * 64 * H
            else:
                assert cache.size == 2 * (n_seq // max(int(g1), 1)) * n_kv * P * hd
            cache_all = put("cache_all", np.zeros(cache.size + 2 * band_rows * hd), np.float16)
        self._chk(self.lib.rk_debug_attn(self.h, C.byref(c)))
        del keep
        res = {}
        for k, _ in RkDebugAttnCall._fields_:
            if k.startswith("out_") and k != "out_all" and k != "out_rows":
                v = getattr(c, k)
                res[k[4:]] = v if isinstance(v, int) else tuple(v)
        if not plan_only:
            res.update(out=out_all, cache=cache_all)
        return res

    def debug_rows(self, op: int, *, ins=(), outs=(), band=256, n_steps=1, plan_only=False, check=True, **params) -> dict:
        """One launch of a row kernel or state machine through rk_debug_rows (include/rk_engine.h).  ins: per input None, an array
        (no bands) or (whole array, interior offset in ELEMENTS); outs: per output the pre-filled interior array.  params: the call's
        int / float fields by name.  Returns "grid", "tparam", "variant", "rc" and, unless plan_only, "all": per output a byte array
        [n_steps, band + bytes + band] - the whole device allocations after every launch.  check=False: a refusal is returned as rc
        (the outputs then still hold what the caller gave) instead of raised."""
        c = RkDebugRowsCall()
        c.op, c.n_steps, c.plan_only = op, n_steps, int(plan_only)
        for k, v in params.items():
            assert k in dict(RkDebugRowsCall._fields_) and k not in ("in_", "out"), k
            setattr(c, k, v)
        keep, alls = [], []
        for i, a in enumerate(ins):
            if a is None:
                continue
            a, off = a if isinstance(a, tuple) else (a, 0)
            a = np.ascontiguousarray(a)
            keep.append(a)
            c.in_[i].data, c.in_[i].bytes, c.in_[i].off = a.ctypes.data, a.nbytes, off * a.itemsize
        for i, a in enumerate(outs):
            if a is None:
                alls.append(None)
                continue
            a = np.ascontiguousarray(a)
            whole = np.full((n_steps, a.nbytes + 2 * band), DEBUG_SENTINEL, np.uint8)      # (a refused call leaves the sentinel everywhere)
            keep.append(a)
            alls.append(whole)
            c.out[i].interior, c.out[i].bytes, c.out[i].band, c.out[i].all = a.ctypes.data, a.nbytes, band, whole.ctypes.data
        rc = self.lib.rk_debug_rows(self.h, C.byref(c))
        if check:
            self._chk(rc)
        del keep
        res = {"rc": rc, "grid": tuple(c.out_grid), "tparam": c.out_tparam, "variant": c.out_variant}
        if not plan_only:
            res["all"] = alls
        return res

    def debug_draft_steps(self, *, n_slots: int, g1: int, script, state, max_admit=0, max_tokens=0, band=256, check=True) -> dict:
        """A drafting session's accept machine and proposer through rk_debug_draft_steps (include/rk_engine.h).  script: int32
        [n_steps, rec] (the header's record layout); state: the 14 initial int32 arrays in DRAFT_ARRAYS' order.  Returns "rc" and
        "all": per array a byte array [n_steps, band + bytes + band], the whole device allocation after every step (sentinel bytes
        where a refused call launched nothing).  check=False: a refusal is returned as rc instead of raised."""
        script = np.ascontiguousarray(script, dtype=np.int32)
        assert script.ndim == 2 and len(state) == len(DRAFT_ARRAYS)
        c = RkDebugDraftStepsCall()
        c.n_slots, c.g1, c.n_steps, c.max_admit, c.max_tokens = n_slots, g1, script.shape[0], max_admit, max_tokens
        c.script, c.script_ints = script.ctypes.data, script.size
        keep, alls = [script], []
        for i, a in enumerate(state):
            a = np.ascontiguousarray(a, dtype=np.int32)
            whole = np.full((script.shape[0], a.nbytes + 2 * band), DEBUG_SENTINEL, np.uint8)
            keep.append(a)
            alls.append(whole)
            c.state[i].interior, c.state[i].bytes, c.state[i].band, c.state[i].all = a.ctypes.data, a.nbytes, band, whole.ctypes.data
        rc = self.lib.rk_debug_draft_steps(self.h, C.byref(c))
        if check:
            self._chk(rc)
        del keep
        return {"rc": rc, "all": alls}

    def debug_xattn_chain(self, *, M: int, Ld: int, H: int, d: int, seq_off, x=None, wq=None, wk=None, wv=None, enc=None, row0=0, row_seq=None,
                          rowscale=None, ssq_in=None, ctx=None, ldo=0, band_rows=8, fuse_asked=True, ws_fill=0, plan_only=False) -> dict:
        """The decoder's query-side cross-attention chain through rk_debug_xattn_chain (include/rk_engine.h).  x [M, ldx], wq / wk / wv
        [H hd, d] (hd = the engine's head width, 64 or 128), enc [band_rows + T + band_rows, d] (the caller's bands), ctx [M, ldo] (the pre-filled interior) or None: fp16.
        Returns the plan fields and, unless plan_only, the whole device allocations after the call: "qk" [band_rows + M + band_rows,
        H, d], "ctx" [band_rows + M + band_rows, ldo], and per block of the row loop "part" [n_blocks, band_rows H d + R nch H d +
        band_rows H d], "stat" [n_blocks, band_rows H 2 + R nch H 2 + band_rows H 2] fp32 and "xctx" [n_blocks, band_rows + R + band_rows,
        H d], R = min(block_rows, M).  The host buffers hold sentinel bytes before the call; a refused call raises RkError with them
        in its `outputs` attribute (a call that launched nothing leaves them as they were)."""
        c = RkDebugXattnChainCall()
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int32)
        hd = 128 if int(getattr(self.desc, "d_kv", 64)) == 128 else 64
        ldo = ldo or hd * H
        c.M, c.Ld, c.H, c.d, c.n_seq, c.row0, c.ldo, c.band_rows = M, Ld, H, d, seq_off.size - 1, row0, ldo, band_rows
        c.fuse_asked, c.ws_fill, c.seq_off = int(fuse_asked), ws_fill, seq_off.ctypes.data
        keep = [seq_off]

        def put(field, a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            setattr(c, field, a.ctypes.data)
            return a

        def sentinel(shape, dt):
            return np.frombuffer(bytes([DEBUG_SENTINEL]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()

        a = put("row_seq", row_seq, np.int32)
        if a is not None:
            c.n_row_seq = a.size
        if x is not None:
            x = put("x", x, np.float16)
            assert x.ndim == 2 and x.shape[0] == M
            c.ldx = x.shape[1]
        for name, w in (("wq", wq), ("wk", wk), ("wv", wv)):
            w = put(name, w, np.float16)
            assert w is None or w.shape == (hd * H, d)
        if enc is not None:
            enc = put("enc", enc, np.float16)
            assert enc.ndim == 2 and enc.shape[1] == d and enc.shape[0] >= 2 * band_rows
            c.enc_rows = enc.shape[0] - 2 * band_rows
        a = put("rowscale", rowscale, np.float32)
        assert a is None or a.size == M
        a = put("ssq_in", ssq_in, np.float32)
        if a is not None:
            assert a.ndim == 2 and a.shape[0] == M
            c.nb_in = a.shape[1]
        a = put("ctx", ctx, np.float16)
        assert a is None or a.shape == (M, ldo)

        def fields():
            res = {}
            for k, _ in RkDebugXattnChainCall._fields_:
                if k.startswith("out_"):
                    v = getattr(c, k)
                    res[k[4:]] = v if isinstance(v, (int, float)) else tuple(tuple(u) if hasattr(u, "__len__") else u for u in v)
            return res

        c.plan_only = 1                                     # the row loop's block size decides the size of the outputs
        rc = self.lib.rk_debug_xattn_chain(self.h, C.byref(c))
        if plan_only:
            self._chk(rc)
            return fields()
        # (a call the plan already refuses is issued all the same, with one-block buffers: it must refuse again and touch nothing)
        R, nb, nch, Hd = (1, 1, 1, H * max(d, 1)) if rc else (min(c.out_block_rows, M), c.out_n_blocks, c.out_nch, H * d)
        c.plan_only = 0
        outs = dict(qk=put("qk_all", sentinel((M + 2 * band_rows, H, max(d, 1)), np.float16), np.float16),
                    part=put("part_all", sentinel((nb, R * nch * Hd + 2 * band_rows * Hd), np.float32), np.float32),
                    stat=put("stat_all", sentinel((nb, R * nch * H * 2 + 2 * band_rows * H * 2), np.float32), np.float32),
                    xctx=put("xctx_all", sentinel((nb, R + 2 * band_rows, Hd), np.float16), np.float16),
                    ctx=put("ctx_all", sentinel((M + 2 * band_rows, ldo), np.float16), np.float16))
        try:
            self._chk(self.lib.rk_debug_xattn_chain(self.h, C.byref(c)))
        except RkError as err:
            err.outputs = outs
            raise
        del keep
        res = fields()
        res.update(outs)
        return res

    def debug_read(self, name: str, n_floats: int) -> np.ndarray:
        out = np.empty(n_floats, dtype=np.float32)
        got = self.lib.rk_debug_read(self.h, name.encode(), out.ctypes.data_as(_f32p), n_floats)
        if got < 0:
            self._chk(int(got))
        return out[:got]

    def debug_sample(self, logits: np.ndarray, temperature: float, top_k: int, top_p: float, seeds, index, check=True):
        """sample_rows_kernel alone through rk_debug_sample (include/rk_engine.h).  logits: fp32 [logit_rows, V]; seeds (uint64) and
        index (int32), one per row of the call: row r draws from logits row r % logit_rows.  -> (token, kept after top-k, kept after
        top-p), int32 [rows] each.  check=False: a refusal is returned as its code instead of raised."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        assert logits.ndim == 2
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        assert seeds.size == index.size
        tok, kk, kp = (np.full(seeds.size, -1, np.int32) for _ in range(3))
        q = RkDebugSampleCall()
        q.rows, q.logit_rows, q.V = seeds.size, logits.shape[0], logits.shape[1]
        q.temperature, q.top_k, q.top_p = float(temperature), int(top_k), float(top_p)
        q.logits, q.seeds, q.index = logits.ctypes.data, seeds.ctypes.data, index.ctypes.data
        q.out_token, q.out_kept_k, q.out_kept_p = tok.ctypes.data, kk.ctypes.data, kp.ctypes.data
        rc = self.lib.rk_debug_sample(self.h, C.byref(q))
        if not check and rc != 0:
            return rc
        self._chk(rc)
        return tok, kk, kp

    def graph_stats(self) -> dict:
        """The decoder graph table and its counters (rk_debug_graph_stats): n_keys, n_ready, max_keys, and since the engine was
        created eager, captures, replays, failed, evictions."""
        st = RkDebugGraphStats()
        self._chk(self.lib.rk_debug_graph_stats(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in RkDebugGraphStats._fields_}

    def buffers(self) -> dict:
        """The grown device buffers and their move counters (rk_debug_buffers): per name of BUFFER_NAMES {"addr", "cap"} (device
        address, 0 before the first allocation; capacity in elements), and amax_gen, kv_gen, lkv_gen.  Host state only."""
        b = RkDebugBuffers()
        self._chk(self.lib.rk_debug_buffers(self.h, C.byref(b)))
        out = {n: {"addr": int(b.addr[i]), "cap": int(b.cap[i])} for i, n in enumerate(BUFFER_NAMES)}
        out.update((k, int(getattr(b, k))) for k in ("amax_gen", "kv_gen", "lkv_gen"))
        return out


class RkLlamaEngine(RkEngine):
    """Decoder-only engine (rk_llama_*): prefill + last-position logits.  Shares weight loading, options, profiling and
    lifetime with RkEngine; the T5 entry points refuse it."""

    def __init__(self, dims, device: int = 0, max_tokens: int = 16384, max_seqs: int = 16, weight_fp8: bool = False):
        self.lib = load_library()
        self.dims = dims
        self.weight_fp8 = bool(weight_fp8)
        self.desc = RkLlamaDesc(vocab=dims.vocab, hidden=dims.hidden, n_heads=dims.n_heads, n_kv_heads=dims.n_kv_heads,
                                head_dim=dims.head_dim, intermediate=dims.intermediate, n_layers=dims.n_layers,
                                tied_head=int(dims.tied_head), eps=dims.eps, rope_theta=dims.rope_theta,
                                max_tokens=max_tokens, max_seqs=max_seqs)
        h = C.c_void_p()
        rc = self.lib.rk_llama_create(C.byref(self.desc), device, C.byref(h))
        if rc != 0:
            raise RkError(rc, (self.lib.rk_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self.comm_rank, self.comm_world = 0, 1
        if self.weight_fp8:                                           # FP8 step weights (opt-in, lossy): before the first tensor is loaded
            self._chk(self.lib.rk_llama_set_weight_fp8(self.h, 1))
        if getattr(dims, "rope_scaling", None) is not None:          # rope type llama3: before finalize builds the rotary tables
            f, lo, hi, orig = dims.rope_scaling
            self._chk(self.lib.rk_llama_set_rope_scaling(self.h, float(f), float(lo), float(hi), int(orig)))
        if getattr(dims, "qkv_bias", False):                          # Qwen2 family: before the first tensor is loaded
            self._chk(self.lib.rk_llama_set_qkv_bias(self.h, 1))
        if getattr(dims, "qk_norm", False):                           # Qwen3 family: the q / k head norm, before finalize
            self._chk(self.lib.rk_llama_set_qk_norm(self.h, 1))
        if getattr(dims, "sliding_window", 0) > 0:                    # Mistral family: the attention's window, before finalize
            self._chk(self.lib.rk_llama_set_sliding_window(self.h, int(dims.sliding_window)))

    def greedy1(self, seqs: Sequence[Sequence[int]]) -> np.ndarray:
        tok, off = pack_ragged(seqs)
        out = np.empty(len(seqs), dtype=np.int32)
        self._chk(self.lib.rk_llama_greedy1(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                            out.ctypes.data_as(_i32p)))
        return out

    def last_logits(self, seqs: Sequence[Sequence[int]], out_ids: Sequence[int]) -> np.ndarray:
        tok, off = pack_ragged(seqs)
        oi = _i32(out_ids)
        out = np.empty((len(seqs), len(oi)), dtype=np.float32)
        self._chk(self.lib.rk_llama_last_logits(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                                oi.ctypes.data_as(_i32p), len(oi), out.ctypes.data_as(_f32p)))
        return out

    def set_sampling(self, temperature: float, top_k: int, top_p: float):
        """rk_llama_set_sampling: temperature 0 = off (greedy), top_k 0 = off, top_p 1 = off.  Only the calls that pass seeds
        sample; a session latches the setting at its open."""
        self._chk(self.lib.rk_llama_set_sampling(self.h, float(temperature), int(top_k), float(top_p)))

    def generate(self, seqs: Sequence[Sequence[int]], max_new: int, eos_ids: Sequence[int], pad_id: int,
                 max_total: int = 0, seeds: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, int]:
        """Greedy continuation of every prompt (rk_llama_generate: the prefill once, then one KV-cached row per sequence and
        step) -> (tokens [B, max_new], columns produced).  A row finishes at one of `eos_ids` (at most 8) or, with max_total >
        0, at that total length; finished rows emit pad_id.  seeds (one 64-bit seed per prompt): rk_llama_generate_sampled - every
        row draws from its own stream under set_sampling's parameters (greedy while sampling is off)."""
        tok, off = pack_ragged(seqs)
        eos = _i32(list(eos_ids))
        out = np.empty((len(seqs), max_new), dtype=np.int32)
        steps = C.c_int32(0)
        if seeds is not None:
            sd = _seeds(seeds, len(seqs))
            self._chk(self.lib.rk_llama_generate_sampled(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                                         int(max_new), int(max_total), eos.ctypes.data_as(_i32p), len(eos), int(pad_id),
                                                         out.ctypes.data_as(_i32p), C.byref(steps), sd.ctypes.data_as(_P(C.c_uint64))))
            return out, int(steps.value)
        self._chk(self.lib.rk_llama_generate(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs), int(max_new),
                                             int(max_total), eos.ctypes.data_as(_i32p), len(eos), int(pad_id),
                                             out.ctypes.data_as(_i32p), C.byref(steps)))
        return out, int(steps.value)

    def session(self, n_slots: int, max_len: int, max_new_cap: int, eos_ids: Sequence[int], pad_id: int,
                draft: int = 0, ngram: Tuple[int, int] = (1, 3)) -> "LlamaSession":
        """A decoding session (rk_llama_session_*): `n_slots` cache slots of `max_len` positions, prompts admitted into free
        slots while the others decode.  A context manager; one per engine, and generate / greedy1 / last_logits are refused
        while it is open.  draft = Kd in 1..7 (rk_llama_session_open_draft): Kd extra rows per slot and step fed with tokens
        drafted by n-gram lookup (ngram = (min, max) lengths) in the request's own prompt and output - the same tokens in fewer
        steps; n_slots * (Kd + 1) <= max_seqs.  draft = 0 launches exactly what it always did."""
        return LlamaSession(self, n_slots, max_len, max_new_cap, eos_ids, pad_id, draft=draft, ngram=ngram)


class LlamaSession:
    """The five session calls of one RkLlamaEngine.  `busy` is the set of slots that hold a request (decoding, or finished and
    not yet read)."""

    def __init__(self, eng: RkLlamaEngine, n_slots: int, max_len: int, max_new_cap: int, eos_ids: Sequence[int], pad_id: int,
                 draft: int = 0, ngram: Tuple[int, int] = (1, 3)):
        self.eng, self.n_slots, self.max_len, self.max_new_cap = eng, int(n_slots), int(max_len), int(max_new_cap)
        self.draft, self.ngram = int(draft), (int(ngram[0]), int(ngram[1]))
        eos = _i32(list(eos_ids))
        self.is_open = False
        if self.draft == 0:                              # the plain entry point, as ever
            eng._chk(eng.lib.rk_llama_session_open(eng.h, self.n_slots, self.max_len, self.max_new_cap, eos.ctypes.data_as(_i32p),
                                                   len(eos), int(pad_id)))
        else:
            eng._chk(eng.lib.rk_llama_session_open_draft(eng.h, self.n_slots, self.max_len, self.max_new_cap, eos.ctypes.data_as(_i32p),
                                                         len(eos), int(pad_id), self.draft, self.ngram[0], self.ngram[1]))
        self.is_open = True
        self.busy = set()
        self.steps = 0                                   # steps issued so far (every step decodes all n_slots rows)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if self.is_open and getattr(self.eng, "h", None):
            self.is_open = False
            self.eng._chk(self.eng.lib.rk_llama_session_close(self.eng.h))

    def free_slots(self):
        return [s for s in range(self.n_slots) if s not in self.busy]

    def admit(self, seqs: Sequence[Sequence[int]], slots: Sequence[int], max_new: Sequence[int],
              seeds: Optional[Sequence[int]] = None) -> None:
        """ONE prefill of `seqs` into the free slots `slots`; prompt b generates up to max_new[b] tokens.  seeds (one per prompt):
        rk_llama_session_admit_sampled, the admit of a session opened while sampling was on."""
        if not (len(seqs) == len(slots) == len(max_new)):
            raise ValueError("admit: seqs, slots and max_new must have one entry per prompt")
        tok, off = pack_ragged(seqs)
        sl, mn = _i32(list(slots)), _i32(list(max_new))
        if seeds is not None:
            sd = _seeds(seeds, len(seqs))
            self.eng._chk(self.eng.lib.rk_llama_session_admit_sampled(self.eng.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p),
                                                                      sl.ctypes.data_as(_i32p), mn.ctypes.data_as(_i32p), len(seqs),
                                                                      sd.ctypes.data_as(_P(C.c_uint64))))
        else:
            self.eng._chk(self.eng.lib.rk_llama_session_admit(self.eng.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p),
                                                              sl.ctypes.data_as(_i32p), mn.ctypes.data_as(_i32p), len(seqs)))
        self.busy.update(int(s) for s in sl)

    def run(self, max_steps: int = 1 << 30):
        """Steps until a slot has newly finished (or nothing is active, or max_steps) -> (finished slots, steps issued)."""
        fin = np.empty(self.n_slots, dtype=np.int32)
        n, steps = C.c_int32(0), C.c_int32(0)
        self.eng._chk(self.eng.lib.rk_llama_session_run(self.eng.h, int(max_steps), fin.ctypes.data_as(_i32p), C.byref(n), C.byref(steps)))
        self.steps += int(steps.value)
        return [int(s) for s in fin[:n.value]], int(steps.value)

    def stats(self) -> dict:
        """rk_llama_session_stats: steps issued by run() since the open, the tokens those steps emitted, and per slot the steps its
        current request was active in and its output column."""
        st, tk = C.c_int64(0), C.c_int64(0)
        ss, sc = np.zeros(self.n_slots, dtype=np.int32), np.zeros(self.n_slots, dtype=np.int32)
        self.eng._chk(self.eng.lib.rk_llama_session_stats(self.eng.h, C.byref(st), C.byref(tk), ss.ctypes.data_as(_i32p), sc.ctypes.data_as(_i32p)))
        return {"steps": int(st.value), "tokens": int(tk.value), "slot_steps": ss, "slot_cols": sc}

    def set_drafts(self, slot: int, tokens: Optional[Sequence[int]]) -> None:
        """debug (rk_debug_session_drafts): the slot's drafts come from this continuation table, indexed by output column, in place
        of the lookup; None: back to the lookup."""
        if tokens is None:
            self.eng._chk(self.eng.lib.rk_debug_session_drafts(self.eng.h, int(slot), None, 0))
            return
        t = _i32(list(tokens))
        self.eng._chk(self.eng.lib.rk_debug_session_drafts(self.eng.h, int(slot), t.ctypes.data_as(_i32p), len(t)))

    def read(self, slot: int) -> np.ndarray:
        """The finished slot's new tokens (its EOS included); the slot is free afterwards."""
        out = np.empty(self.max_new_cap, dtype=np.int32)
        n = C.c_int32(0)
        self.eng._chk(self.eng.lib.rk_llama_session_read(self.eng.h, int(slot), out.ctypes.data_as(_i32p), len(out), C.byref(n)))
        self.busy.discard(int(slot))
        return out[:n.value].copy()


def rel_bucket(rel: int, bidirectional: bool, num_buckets: int = 32, max_distance: int = 128) -> int:
    """The C++ restatement of hf: modeling_t5.py:216-262 that builds the device bias tables (host-only call)."""
    return load_library().rk_rel_bucket(int(rel), int(bidirectional), num_buckets, max_distance)
