"""The rk_debug_* side of the ctypes binding (include/rk_engine.h): the call structs, their constants and, as the mixin DebugCalls,
the debug methods of RkEngine.  _engine.py imports every name here, keeps the one ABI table and is what everything else imports
from; this module imports nothing of _engine.py.
"""
from __future__ import annotations

import ctypes as C
from functools import partial
from typing import Optional, Tuple

import numpy as np


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


class RkDebugKv8StepCall(C.Structure):
    """rk_debug_kv8_step_call of include/rk_engine.h, field for field."""
    _fields_ = [(n, C.c_int) for n in ("n_seq", "H", "n_kv", "P", "ld", "max_pos", "g1", "mode", "plan_only")] + [("qk_eps", C.c_float)] + \
               [(n, C.c_void_p) for n in ("qkv", "pos", "cos_t", "sin_t", "qkv_bias", "qk_norm", "live", "cache")] + \
               [("ctx", RkDebugRowsOut), ("part", RkDebugRowsOut), ("cache_out", RkDebugRowsOut)] + \
               [(n, C.c_int) for n in ("out_R", "out_nch", "out_pe")]


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


_P = C.POINTER
_f32p = _P(C.c_float)


def _sentinel(shape, dt) -> np.ndarray:
    """an array of `shape` and dtype `dt` whose every byte is DEBUG_SENTINEL: what a refused call must leave as it was"""
    return np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, DEBUG_SENTINEL, np.uint8).view(dt).reshape(shape)


def _put(call, keep: list, field: str, a, dt):
    """`a` (or None) as a contiguous array of dtype `dt`: its address into call.<field>, the array into `keep` (alive over the call)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dt)
    keep.append(a)
    setattr(call, field, a.ctypes.data)
    return a


def _banded_outs(slots, arrays, dt, n_steps: int, band: int, keep: list) -> list:
    """Fills the rk_debug_rows_out `slots` from the interiors `arrays` (None: unused) -> per array the byte array [n_steps, band +
    bytes + band] its whole allocation is read back into after every step (sentinel bytes: a refused call leaves them everywhere)"""
    alls = []
    assert len(arrays) <= len(slots)
    for slot, a in zip(slots, arrays):
        if a is None:
            alls.append(None)
            continue
        a = np.ascontiguousarray(a, dtype=dt)
        alls.append(_sentinel((n_steps, a.nbytes + 2 * band), np.uint8))
        keep.append(a)
        slot.interior, slot.bytes, slot.band, slot.all = a.ctypes.data, a.nbytes, band, alls[-1].ctypes.data
    return alls


def _plain(v):
    return v if isinstance(v, (int, float)) else tuple(_plain(u) for u in v)


def _out_fields(call, prefix: str = "out_", skip=()) -> dict:
    """the `prefix` fields of a call struct as a dict without the prefix: ints and floats as they are, arrays as (nested) tuples"""
    return {k[len(prefix):]: _plain(getattr(call, k)) for k, _ in call._fields_ if k.startswith(prefix) and k not in skip}


class DebugCalls:
    """RkEngine's debug_* / gemm_bench / graph_stats / buffers methods (the rk_debug_* entry points of include/rk_engine.h).  A
    mixin: it uses the engine's lib, h, desc and _chk."""


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
        if plan_only:
            # the plan reads shapes, strides and WHICH operands are there, never their bytes (rk_debug_gemm_ex returns in front of
            # its extent checks): one word stands for every array, so a sweep over M costs no M-sized allocation
            q = RkDebugGemmCall()
            q.epi, q.family, q.M, q.N, q.K, q.lda, q.ldw, q.ldc, q.c_off = epi, family, M, N, K, lda, ldw, ldc, c_off
            q.n_split, q.split_stride, q.batch, q.bsA, q.bsW, q.bsC = n_split, split_stride, batch, bsA, bsW, bsC
            word = np.zeros(4, dtype=np.float32)
            if rowscale is not None:
                q.rowscale = word.ctypes.data
            if ssq_in is not None:
                q.ssq_in, q.nb_in, q.factors_kernel = word.ctypes.data, np.shape(ssq_in)[1], int(factors_kernel)
            if producer:
                q.xraw_out = q.ssq_out = word.ctypes.data
            q.plan_only = 1
            self._chk(getattr(self.lib, entry)(self.h, C.byref(q)))
            return _out_fields(q)
        if c_in is None:
            nsb = -(-N // n_split) if n_split else 1
            c_elems = c_off + (batch - 1) * bsC + (nsb - 1) * split_stride + M * ldc
            c_in = _sentinel(c_elems * per, dt)
        c_in = np.ascontiguousarray(c_in, dtype=dt).reshape(-1)
        c_elems = c_in.size // per
        band = DEBUG_BAND_ROWS * ldc
        q = RkDebugGemmCall()
        q.epi, q.family, q.M, q.N, q.K, q.lda, q.ldw, q.ldc = epi, family, M, N, K, lda, ldw, ldc
        q.A, q.a_elems, q.W, q.w_elems = a16.ctypes.data, a16.size, w16.ctypes.data, w16.size
        q.C, q.c_elems, q.c_off, q.band_rows = c_in.ctypes.data, c_elems, c_off, DEBUG_BAND_ROWS
        c_out = np.zeros((2 * band + c_elems) * per, dtype=dt)
        q.C_out = c_out.ctypes.data
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
            xlab = _sentinel(M, np.float32)
            q.labels, q.xlab = labels.ctypes.data, xlab.ctypes.data
        self._chk(getattr(self.lib, entry)(self.h, C.byref(q)))
        out = _out_fields(q)
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

    def debug_kv8_quant(self, x16: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The FP8 K / V cache's quantiser on host vectors (rk_debug_kv8_quant; the format: include/rk_engine.h at rk_llama_set_kv_fp8).
        x16: fp16 [n, 128].  Returns (e4m3fn bytes [n, 128] uint8, exponents [n] int8, the dequantised fp16 vectors [n, 128])."""
        x16 = np.ascontiguousarray(x16, dtype=np.float16)
        assert x16.ndim == 2 and x16.shape[1] == 128
        n = x16.shape[0]
        q, ex, deq = np.zeros((n, 128), np.uint8), np.zeros(n, np.int8), np.zeros((n, 128), np.float16)
        self._chk(self.lib.rk_debug_kv8_quant(self.h, x16.ctypes.data_as(_P(C.c_uint16)), n, q.ctypes.data_as(_P(C.c_uint8)),
                                              ex.ctypes.data_as(_P(C.c_int8)), deq.ctypes.data_as(_P(C.c_uint16))))
        return q, ex, deq

    def debug_kv8_step(self, *, mode: int, qkv, pos, cos, sin, cache, H: int, n_kv: int, P: int, qkv_bias=None, qk_norm=None, qk_eps=0.0,
                       g1=0, live=None, band=256, fill=0.0, plan_only=False) -> dict:
        """One step's attention of an FP8-cache engine through rk_debug_kv8_step (include/rk_engine.h).  qkv fp16 [n_seq, ld]; cache
        fp16, flat, K then V ([2][n_seq / g1][n_kv][P][128]); mode 0 = bytes, 1 = rounded fp16.  Returns R, nch, pe and, unless
        plan_only, the whole device allocations after the call as byte arrays "ctx", "part", "cache" (band + interior + band each)
        and "band"; the interiors of ctx and part are pre-filled with `fill`."""
        qkv = np.ascontiguousarray(qkv, dtype=np.float16)
        n_seq, ld = qkv.shape
        c = RkDebugKv8StepCall()
        c.n_seq, c.H, c.n_kv, c.P, c.ld, c.g1, c.mode, c.plan_only = n_seq, H, n_kv, P, ld, int(g1), int(mode), 1
        self._chk(self.lib.rk_debug_kv8_step(self.h, C.byref(c)))
        res = _out_fields(c)
        if plan_only:
            return res
        c.plan_only = 0
        keep = [qkv]
        put = partial(_put, c, keep)
        c.qkv = qkv.ctypes.data
        put("pos", pos, np.int32)
        cos, sin = put("cos_t", cos, np.float32), put("sin_t", sin, np.float32)
        assert cos.ndim == 2 and cos.shape[1] == 64 and sin.shape == cos.shape
        c.max_pos = cos.shape[0]
        put("qkv_bias", qkv_bias, np.float32)
        if qk_norm is not None:
            put("qk_norm", qk_norm, np.float32)
            c.qk_eps = float(qk_eps)
        put("live", live, np.int32)
        rows = n_seq // max(int(g1), 1)
        plane = rows * n_kv * P * 128
        assert put("cache", cache, np.float16).size == 2 * plane
        cache_bytes = 4 * plane if mode else 2 * plane + 2 * rows * n_kv * res["pe"]
        outs = [np.full((n_seq, H * 128), fill, np.float16), np.full(n_seq * H * res["nch"] * 132, fill, np.float32),
                np.zeros(cache_bytes, np.uint8)]
        alls = _banded_outs([c.ctx, c.part, c.cache_out], outs, None, 1, band, keep)
        self._chk(self.lib.rk_debug_kv8_step(self.h, C.byref(c)))
        res.update(ctx=alls[0][0], part=alls[1][0], cache=alls[2][0], band=band)
        return res

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
                c_in = _sentinel(n_out * c_elems, dt)
            c_in = np.ascontiguousarray(c_in, dtype=dt).reshape(-1)
            assert c_in.size == n_out * c_elems
            if c_out is None:
                c_out = _sentinel(n_out * (2 * band + c_elems), dt)
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
        out = _out_fields(q)
        out.update(("bg_" + k, v) for k, v in _out_fields(q, "bg_out_").items())
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
        put = partial(_put, c, keep)
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
        res = _out_fields(c, skip=("out_all", "out_rows"))
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
        keep = []
        for i, a in enumerate(ins):
            if a is None:
                continue
            a, off = a if isinstance(a, tuple) else (a, 0)
            a = np.ascontiguousarray(a)
            keep.append(a)
            c.in_[i].data, c.in_[i].bytes, c.in_[i].off = a.ctypes.data, a.nbytes, off * a.itemsize
        alls = _banded_outs(c.out, outs, None, n_steps, band, keep)
        rc = self.lib.rk_debug_rows(self.h, C.byref(c))
        if check:
            self._chk(rc)
        res = dict(_out_fields(c, skip=("out_scale",)), rc=rc)      # (out_scale is an operand of op 3)
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
        keep = [script]
        alls = _banded_outs(c.state, state, np.int32, script.shape[0], band, keep)
        rc = self.lib.rk_debug_draft_steps(self.h, C.byref(c))
        if check:
            self._chk(rc)
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
        put = partial(_put, c, keep)
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

        c.plan_only = 1                                     # the row loop's block size decides the size of the outputs
        rc = self.lib.rk_debug_xattn_chain(self.h, C.byref(c))
        if plan_only:
            self._chk(rc)
            return _out_fields(c)
        # (a call the plan already refuses is issued all the same, with one-block buffers: it must refuse again and touch nothing)
        R, nb, nch, Hd = (1, 1, 1, H * max(d, 1)) if rc else (min(c.out_block_rows, M), c.out_n_blocks, c.out_nch, H * d)
        c.plan_only = 0
        outs = dict(qk=put("qk_all", _sentinel((M + 2 * band_rows, H, max(d, 1)), np.float16), np.float16),
                    part=put("part_all", _sentinel((nb, R * nch * Hd + 2 * band_rows * Hd), np.float32), np.float32),
                    stat=put("stat_all", _sentinel((nb, R * nch * H * 2 + 2 * band_rows * H * 2), np.float32), np.float32),
                    xctx=put("xctx_all", _sentinel((nb, R + 2 * band_rows, Hd), np.float16), np.float16),
                    ctx=put("ctx_all", _sentinel((M + 2 * band_rows, ldo), np.float16), np.float16))
        try:
            self._chk(self.lib.rk_debug_xattn_chain(self.h, C.byref(c)))
        except RuntimeError as err:                         # (_chk's RkError)
            err.outputs = outs
            raise
        res = _out_fields(c)
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
        return _out_fields(st, prefix="")

    def buffers(self) -> dict:
        """The grown device buffers and their move counters (rk_debug_buffers): per name of BUFFER_NAMES {"addr", "cap"} (device
        address, 0 before the first allocation; capacity in elements), and amax_gen, kv_gen, lkv_gen.  Host state only."""
        b = RkDebugBuffers()
        self._chk(self.lib.rk_debug_buffers(self.h, C.byref(b)))
        out = {n: {"addr": int(b.addr[i]), "cap": int(b.cap[i])} for i, n in enumerate(BUFFER_NAMES)}
        out.update((k, int(getattr(b, k))) for k in ("amax_gen", "kv_gen", "lkv_gen"))
        return out
