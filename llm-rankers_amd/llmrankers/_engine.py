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

# the rk_debug_* side of the ABI: its call structs and constants (part of this module's names, as ever) and RkEngine's debug methods
from ._engine_debug import (BUFFER_NAMES, DEBUG_BAND_ROWS, DEBUG_SENTINEL, DRAFT_ARRAYS, GEMM_OUT_DTYPE,  # noqa: F401
                            DebugCalls, RkDebugAttnCall, RkDebugBuffers, RkDebugDraftStepsCall, RkDebugGemmCall,
                            RkDebugGemmChainCall, RkDebugGraphStats, RkDebugKv8StepCall, RkDebugRowsCall, RkDebugRowsIn, RkDebugRowsOut,
                            RkDebugSampleCall, RkDebugXattnChainCall)

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
    "rk_llama_set_kv_fp8": (C.c_int, [C.c_void_p, C.c_int]),
    "rk_llama_greedy1": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p]),
    "rk_llama_last_logits": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _f32p]),
    "rk_llama_qlm": (C.c_int, [C.c_void_p, _i32p, _i32p, C.c_int, _i32p, _f32p]),
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
    "rk_debug_kv8_quant": (C.c_int, [C.c_void_p, _P(C.c_uint16), C.c_int, _P(C.c_uint8), _P(C.c_int8), _P(C.c_uint16)]),
    "rk_debug_kv8_step": (C.c_int, [C.c_void_p, _P(RkDebugKv8StepCall)]),
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


class RkEngine(DebugCalls):
    """One engine = one MI355X.  Thin object wrapper; all compute happens in the HIP library.  The debug_* / gemm_bench /
    graph_stats / buffers methods are DebugCalls' (_engine_debug.py)."""

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


class RkLlamaEngine(RkEngine):
    """Decoder-only engine (rk_llama_*): prefill + last-position logits.  Shares weight loading, options, profiling and
    lifetime with RkEngine; the T5 entry points refuse it."""

    def __init__(self, dims, device: int = 0, max_tokens: int = 16384, max_seqs: int = 16, weight_fp8: bool = False,
                 kv_fp8: bool = False):
        self.lib = load_library()
        self.dims = dims
        self.weight_fp8 = bool(weight_fp8)
        self.kv_fp8 = bool(kv_fp8)
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
        if self.kv_fp8:                                               # FP8 K / V cache of the decoding step (opt-in, lossy): before finalize
            self._chk(self.lib.rk_llama_set_kv_fp8(self.h, 1))
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

    def qlm(self, seqs: Sequence[Sequence[int]], n_labels: Sequence[int]) -> np.ndarray:
        """rk_llama_qlm: float32 [n_seq], the log-likelihood of every sequence's last n_labels[b] tokens given the tokens in front
        of them (natural logarithm, full-vocabulary softmax).  A sequence's score does not depend on what shares its call."""
        if len(n_labels) != len(seqs):
            raise ValueError(f"{len(seqs)} sequences but {len(n_labels)} label counts")
        tok, off = pack_ragged(seqs)
        nl = _i32(n_labels)
        out = np.empty(len(seqs), dtype=np.float32)
        self._chk(self.lib.rk_llama_qlm(self.h, tok.ctypes.data_as(_i32p), off.ctypes.data_as(_i32p), len(seqs),
                                        nl.ctypes.data_as(_i32p), out.ctypes.data_as(_f32p)))
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
