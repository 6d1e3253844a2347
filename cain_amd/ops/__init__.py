"""Python bindings of the hand-written gfx950 kernels (``libcain_kernels.so``).

Every op takes torch tensors living on the GPU and launches on the current
torch stream.  There is no silent eager fallback: if the native library is
missing or fails to load, the ops raise ``NativeOpsUnavailable`` (the engine's
torch-eager path is a separate, explicitly selected backend used on CPU).

Kernel inventory:

=====================  ==========================  =============================
op                     source                      replaces (Ollama/llama.cpp)
=====================  ==========================  =============================
``skinny_gemm``        csrc/gemm.hip               O / gate-up(+act) / down / LM head GEMV,
                       csrc/wgemm.hip              fused RMSNorm, residual epilogue (wgemm: the
                                                   LDS-DMA ring kernel for 64 < M <= 256 rows)
``qkv_rope``           csrc/gemm.hip               QKV GEMV + bias + RoPE + KV-cache append
``gemm_w8``            csrc/gemm_w8.hip            the same GEMMs on fp8 (e4m3) weights, <= 64 rows
``gemm_w8a8``          csrc/wgemm8.hip             fp8 weights x per-row fp8 activations, 16 < M <= 256
``gemm_w4``            csrc/gemm_w4.hip            the same GEMMs on MXFP4 (e2m1 + e8m0) weights, <= 64 rows
``gemm_q4``            csrc/gemm_qstream.hip       the same GEMMs on GGUF Q4_0 / Q4_K blocks (exact values), any M
``gemm_q6``            csrc/gemm_qstream.hip       the same on GGUF Q6_K blocks (a Q4_K_M file's 6-bit tensors), any M
``rmsnorm``            csrc/norm.hip               RMSNorm (standalone; the engine fuses it)
``embed``              csrc/norm.hip               embedding gather (+Gemma scale)
``pool_rows``          csrc/pool.hip               embeddings: final RMSNorm + last / mean pooling of prefill rows
``pool_finish``        csrc/pool.hip               embeddings: mean over the count, L2 normalisation
``attention``          csrc/attention.hip          decode / prefill attention (split-K, in-kernel combine)
``kv_copy_prefix``     csrc/kv_prefix.hip          a slot's cached prompt prefix copied to another slot
``sample``             csrc/sample.hip             repeat-penalty/temperature/top-k/top-p
``logprob_rows``       csrc/logprob.hip            log-softmax, top-n and token logprobs on device
``json_mask``          csrc/grammar.hip            format "json": the JSON grammar as a logit mask on device
``json_advance``       csrc/grammar.hip            the rows' automaton states over the sampled tokens
``stop_advance``       csrc/stopseq.hip            options.stop: stop strings matched over the sampled tokens' bytes
``spec_draft``         csrc/spec.hip              n-gram / given drafts -> K + 1 expanded rows per sequence
``spec_accept``        csrc/spec.hip               commit the longest correct draft prefix (lookup decoding)
``spec_model_rows``    csrc/spec.hip               draft-model mode: the draft model's rows per forward, its tokens
``spec_model_next``                                into the given drafts, ``dvalid`` per cache slot
``spec_dvalid``
``Plan``               csrc/runtime.hip            per-step schedule + hipGraph replay
=====================  ==========================  =============================
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path
from typing import Optional

import torch

HERE = Path(__file__).resolve().parent
# CAIN_KERNELS_LIB: another build of the library (A/B runs of a kernel change on one box)
LIB_PATH = Path(os.environ.get("CAIN_KERNELS_LIB") or HERE / "libcain_kernels.so")

EPI_BF16, EPI_RESID, EPI_F32, EPI_SILU, EPI_GELU, EPI_QKV_ROPE = 0, 1, 2, 3, 4, 5
EPI_KV_FP8 = 0x100  # or-ed into EPI_QKV_ROPE: the KV cache is fp8 e4m3 (csrc/gemm_epi.h)


class NativeOpsUnavailable(RuntimeError):
    pass


class CainGemm(ctypes.Structure):
    """The call record of every GEMM entry (csrc/cain_api.h CainGemm, which says what each entry reads)."""
    _fields_ = ([(f, ctypes.c_void_p) for f in ("W", "sc", "dd", "gain", "xs", "X", "Y", "bias", "slot", "pos", "cos_t",
                                                "sin_t", "kc", "vtc", "ws")]
                + [("ws_bytes", ctypes.c_longlong)]
                + [(f, ctypes.c_int) for f in ("ldx", "K", "N", "M", "ldy", "norm")] + [("eps", ctypes.c_float)]
                + [(f, ctypes.c_int) for f in ("H", "Hkv", "hd", "T_max", "epi", "fmt", "tile0", "waves")])


vp = ctypes.c_void_p
ci = ctypes.c_int
cf = ctypes.c_float

# ---- the records of a plan and of its step (csrc/cain_api.h, csrc/spec.h; CainLayer / CainPlanDesc: csrc/runtime.hip)
LAYER_FIELDS = ("wqkv", "bqkv", "wo", "wgu", "wdown", "sqkv", "so", "sgu", "sdown", "wqkv8", "wo8", "wgu8", "wdown8")
LAYER_FORMATS = ("fqkv", "fo", "fgu", "fdown")  # per-matrix format ids of a GGUF plan, then the split V


class CainLayer(ctypes.Structure):
    _fields_ = [(n, vp) for n in LAYER_FIELDS] + [(n, ci) for n in LAYER_FORMATS] + [("wv", vp), ("sv", vp)]


class CainPlanDesc(ctypes.Structure):
    _fields_ = ([(n, ci) for n in ("n_layers", "d", "H", "Hkv", "hd", "ffn", "V", "act_kind", "T_max", "Mpad", "nsplit",
                                   "waves")]
                + [(n, cf) for n in ("eps", "embed_scale", "attn_scale")]
                + [(n, vp) for n in ("embed", "lm_head", "layers", "kcache", "vtcache")]
                + [("kv_layer_elems", ctypes.c_longlong)]
                + [(n, vp) for n in ("cos_t", "sin_t", "x", "q", "attn", "act", "logits", "part_o", "part_ml",
                                     "counters", "gemm_ws")]
                + [("gemm_ws_bytes", ctypes.c_longlong), ("wfmt", ci), ("lm_head_scale", vp), ("kv8", ci),
                   ("lm_head8", vp), ("x8", vp), ("xs", vp), ("x8_ld", ci), ("q4_gain", ci), ("flm_head", ci)])


class CainRows(ctypes.Structure):
    _fields_ = ([(n, vp) for n in ("tok", "pos", "slot", "n_gen", "max_new", "done", "hist", "gen")]
                + [("ldg", ci), ("sample_params", vp), ("sample_ext", vp)])


class CainLogprob(ctypes.Structure):
    _fields_ = [("topn", vp), ("nmax", ci), ("lp", vp), ("top_id", vp), ("top_lp", vp), ("keep", vp), ("target", vp)]


class CainGrammar(ctypes.Structure):
    _fields_ = [("gram_on", vp), ("gstate", vp), ("piece_off", vp), ("piece_bytes", vp)]


class CainStop(ctypes.Structure):
    _fields_ = [("stop_on", vp), ("sstate", vp), ("stop_len", vp), ("stop_bytes", vp), ("piece_off", vp),
                ("piece_bytes", vp)]


_SPEC_INTS = ("K", "mode", "slots", "lds", "ldv", "ldt", "vocab", "ldg")
_SPEC_PTRS = ("seq", "given", "x_tok", "x_pos", "x_slot", "x_n_gen", "x_max_new", "x_done", "x_hist", "x_gen",
              "x_params", "nd", "draft", "drafted", "accepted", "n_step", "step_tokens")
_SPECD_INTS = ("K", "dvocab", "dbos", "slots", "lds", "ldv", "ldg", "pad_")
_SPECD_PTRS = ("seq", "given", "dvalid", "p0", "nd", "r_tok", "r_pos", "r_slot", "r_n_gen", "r_max_new", "r_done",
               "r_hist", "r_gen", "r_params")


class CainSpec(ctypes.Structure):
    _fields_ = [(n, ci) for n in _SPEC_INTS] + [(n, vp) for n in _SPEC_PTRS]


class CainSpecDraft(ctypes.Structure):
    _fields_ = [(n, ci) for n in _SPECD_INTS] + [(n, vp) for n in _SPECD_PTRS]


class CainPool(ctypes.Structure):
    _fields_ = ([(n, vp) for n in ("gain", "seg_off", "seg_dst", "acc", "cnt", "rinv")] + [("S", ci), ("mode", ci)])


POOL_MEAN, POOL_LAST = 0, 1  # CainPool.mode (csrc/cain_api.h)
POOL_MODES = {"mean": POOL_MEAN, "last": POOL_LAST}


class CainStep(ctypes.Structure):
    """The call record of ``cain_step_run`` / ``cain_step_capture`` (csrc/cain_api.h CainStep, which says what the
    entries refuse).  It holds raw pointers to the other records: whoever fills it keeps those objects alive."""
    _fields_ = ([("plan", vp), ("draft2", vp), ("draft1", vp), ("rows", ctypes.POINTER(CainRows)),
                 ("lp", ctypes.POINTER(CainLogprob)), ("gr", ctypes.POINTER(CainGrammar)),
                 ("st", ctypes.POINTER(CainStop)), ("spec", ctypes.POINTER(CainSpec)),
                 ("spec_draft", ctypes.POINTER(CainSpecDraft)), ("pool", ctypes.POINTER(CainPool))]
                + [(n, ci) for n in ("M", "want_logits", "want_sample")])


# the native size entry of every record
_RECORD_SIZES = ((CainGemm, "cain_gemm_size"), (CainLayer, "cain_layer_size"), (CainPlanDesc, "cain_plan_desc_size"),
                 (CainRows, "cain_rows_size"), (CainLogprob, "cain_logprob_size"), (CainGrammar, "cain_grammar_size"),
                 (CainStop, "cain_stop_size"), (CainSpec, "cain_spec_size"), (CainSpecDraft, "cain_spec_draft_size"),
                 (CainPool, "cain_pool_size"), (CainStep, "cain_step_size"))

_lib: Optional[ctypes.CDLL] = None
_lock = threading.Lock()


def load() -> ctypes.CDLL:
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            if os.environ.get("CAIN_AUTOBUILD", "1") != "0":
                from .. import build
                build.build_kernels()
            if not LIB_PATH.exists():
                raise NativeOpsUnavailable(f"{LIB_PATH} missing: run `python -m cain_amd.build`")
        try:
            real = ctypes.CDLL(str(LIB_PATH))
        except OSError as exc:
            raise NativeOpsUnavailable(f"cannot load {LIB_PATH}: {exc}") from exc
        # an older build loaded for an A/B run (CAIN_KERNELS_LIB) may lack newer entry points: their signatures
        # are skipped (a call to one then fails by name)
        lib = _Lenient(real) if os.environ.get("CAIN_KERNELS_LIB") else real
        if int(real.cain_sample_params_size()) != SAMPLE_BYTES:  # also an A/B build from an older source
            raise NativeOpsUnavailable(f"{LIB_PATH} packs {int(real.cain_sample_params_size())}-byte sampling "
                                       f"options, this package {SAMPLE_BYTES}: rebuild (python -m cain_amd.build)")
        # every record's size, and the sizes and limits of the kernels' per-row states (a build from before a record
        # has no size entry for it and no entry that takes it: a call fails by name)
        sizes = [(rec.__name__, entry, ctypes.sizeof(rec)) for rec, entry in _RECORD_SIZES] + [
            ("JSON_STATE_BYTES", "cain_json_state_size", JSON_STATE_BYTES),
            ("STOP_STATE_BYTES", "cain_stop_state_size", STOP_STATE_BYTES), ("STOP_MAX", "cain_stop_max", STOP_MAX),
            ("STOP_LEN_MAX", "cain_stop_len_max", STOP_LEN_MAX),
            ("SAMPLE_EXT_BYTES", "cain_sample_ext_size", SAMPLE_EXT_BYTES)]
        for name, entry, mine in sizes:
            if hasattr(real, entry) and int(getattr(real, entry)()) != mine:
                raise NativeOpsUnavailable(f"{LIB_PATH}: {name} is {int(getattr(real, entry)())}, this package's is "
                                           f"{mine}: rebuild (python -m cain_amd.build)")
        for entry in ("bf16", "fp8", "mxfp4", "gguf", "fp8a8", "mxfp4a8"):
            getattr(lib, "cain_gemm_" + entry).argtypes = [ctypes.POINTER(CainGemm), vp]
        lib.cain_gemm_w4_ws_bytes.restype = ctypes.c_longlong
        lib.cain_gemm_w4_ws_bytes.argtypes = [ci, ci, ci]
        lib.cain_gemm_w4_split.argtypes = [ci, ci, ci, ci, ctypes.c_longlong]
        lib.cain_gemm_w4_set_split.argtypes = [ci]
        lib.cain_gemm_w4_set_split_cap.argtypes = [ci]
        lib.cain_gemm_w4_set_split_min_quads.argtypes = [ci]
        lib.cain_gemm_w4_set_variant.argtypes = [ci]
        lib.cain_wgemm_set_inline.argtypes = [ci]
        lib.cain_gemm_q4_rows.argtypes = [ci, ci]
        lib.cain_gemm_q6_rows.argtypes = [ci, ci]
        lib.cain_gemm_q_set_tile.argtypes = [ci]
        lib.cain_gemm_q_set_tile.restype = None
        lib.cain_gemm_q_set_tile_nb.argtypes = [ci]
        lib.cain_gemm_q_set_tile_nb.restype = None
        lib.cain_gemm_q_passes.argtypes = [ci, ci, ci, ci]
        lib.cain_wgemm_inline.argtypes = [ci, ci, ci]
        lib.cain_wgemm_get_inline.argtypes = []
        lib.cain_gemm_w4_variant.argtypes = [ci, ci, ci, ci]
        lib.cain_gemm_w4_set_occupancy.argtypes = [ci]
        lib.cain_quant_rows.argtypes = [vp, ci, ci, ci, vp, ci, vp, ci, cf, vp]
        lib.cain_w4a8_set_min_rows.argtypes = [ci]
        lib.cain_w8a8_eligible.argtypes = [ci, ci, ci]
        lib.cain_w8a8_ws_bytes.restype = ctypes.c_longlong
        lib.cain_w8a8_ws_bytes.argtypes = [ci, ci, ci]
        lib.cain_gemm_ws_bytes.restype = ctypes.c_longlong
        lib.cain_gemm_ws_bytes.argtypes = [ci, ci, ci]
        lib.cain_wgemm_set_min_m.argtypes = [ci]
        lib.cain_wgemm_eligible.argtypes = [ci, ci, ci]
        lib.cain_wgemm_set_shape.argtypes = [ci, ci, ci, ci, ci]
        lib.cain_wgemm_plan.argtypes = [ci, ci, ci]
        lib.cain_rmsnorm.argtypes = [vp, ci, vp, vp, ci, ci, ci, cf, vp]
        lib.cain_embed.argtypes = [vp, vp, vp, ci, ci, ci, cf, vp]
        lib.cain_pool_rows.argtypes = [vp, ci, ci, ci, vp, cf, vp, vp, ci, ci, vp, vp, vp, vp]
        lib.cain_pool_finish.argtypes = [vp, vp, vp, ci, ci, ci, vp]
        lib.cain_attention.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp]
        lib.cain_attention_ex.argtypes = ([vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, cf, ci, cf, cf]
                                          + [vp])
        lib.cain_attention_set_ring.argtypes = [ci]
        lib.cain_attention_set_body.argtypes = [ci]
        # (params, ext, stream: the last three of each; ext may be null)
        lib.cain_sample.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        lib.cain_sample_cm.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        lib.cain_sample_lean.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp]
        lib.cain_gemm_set_cmax.argtypes = [vp]
        lib.cain_gemm_set_cmax.restype = None
        lib.cain_gemm_cmax_take.argtypes = []
        lib.cain_sample_set_cm.argtypes = [ci]
        lib.cain_gemm_set_skinny_split.argtypes = [ci]
        lib.cain_sample_ex.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp,
                                       ctypes.c_longlong, vp]
        lib.cain_sample_set_trace.argtypes = [vp]
        lib.cain_sample_ws_bytes.restype = ctypes.c_longlong
        lib.cain_sample_ws_bytes.argtypes = [ci]
        lib.cain_plan_create.restype = vp
        lib.cain_plan_create.argtypes = [vp]
        lib.cain_plan_destroy.argtypes = [vp]
        lib.cain_plan_last_failure.restype = ctypes.c_char_p
        lib.cain_step_run.argtypes = [ctypes.POINTER(CainStep), vp]
        lib.cain_step_capture.restype = vp
        lib.cain_step_capture.argtypes = [ctypes.POINTER(CainStep), ci, vp, ctypes.POINTER(ci)]
        lib.cain_graph_launch.argtypes = [vp, vp]
        lib.cain_graph_destroy.argtypes = [vp]
        lib.cain_set_cu_budget.argtypes = [ci]
        lib.cain_cu_mask.argtypes = [ci, ci, ctypes.POINTER(ctypes.c_uint32), ci]
        lib.cain_stream_create_cu_limited.restype = vp
        lib.cain_stream_create_cu_limited.argtypes = [ci]
        lib.cain_stream_destroy.argtypes = [vp]
        lib.cain_kv_copy_prefix.argtypes = [vp, vp, ctypes.c_longlong, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp]
        lib.cain_logprob_rows.argtypes = [vp, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        lib.cain_logprob_pre.argtypes = [vp, ci, ci, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp]
        lib.cain_logprob_chosen.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp, vp]
        lib.cain_logprob_keep_bytes.restype = ctypes.c_longlong
        lib.cain_logprob_keep_bytes.argtypes = [ci]
        lib.cain_json_mask.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        lib.cain_json_advance.argtypes = [ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        lib.cain_stop_advance.argtypes = [ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.cain_spec_draft.argtypes = [vp, ci, ci] + [vp] * 9
        lib.cain_spec_accept.argtypes = [vp, ci, ci] + [vp] * 8 + [ci, vp, vp]
        lib.cain_spec_model_rows.argtypes = [vp, ci, ci] + [vp] * 9
        lib.cain_spec_model_next.argtypes = [vp, ci, ci, ci, vp, vp, vp]
        lib.cain_spec_dvalid.argtypes = [vp, ci, ci, vp, vp, vp]
        if os.environ.get("CAIN_WGEMM_INLINE") and hasattr(real, "cain_wgemm_set_inline"):  # A/B runs
            real.cain_wgemm_set_inline(int(os.environ["CAIN_WGEMM_INLINE"]))
        if os.environ.get("CAIN_SAMPLE_CM"):  # A/B runs (set_sample_cm)
            real.cain_sample_set_cm(int(os.environ["CAIN_SAMPLE_CM"]))
        _lib = real
        return real


class _Lenient:
    """Signature setter over a CDLL that ignores symbols the library does not export."""

    class _Sink:
        def __setattr__(self, k, v):
            pass

    def __init__(self, lib):
        object.__setattr__(self, "_lib", lib)

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            return _Lenient._Sink()


def available() -> bool:
    try:
        load()
        return True
    except NativeOpsUnavailable:
        return False


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc})")


def step_run(step: CainStep, stream) -> None:
    """Enqueue one step (``cain_step_run``) on ``stream`` (a native handle)."""
    lib = load()
    rc = lib.cain_step_run(ctypes.byref(step), stream)
    if rc != 0:
        where = lib.cain_plan_last_failure()
        raise RuntimeError(f"cain_step_run failed rc={rc}" + (f" at {where.decode()}" if where else ""))


def step_capture(step: CainStep, steps: int, stream) -> int:
    """``steps`` such steps recorded on ``stream`` into one executable graph (``cain_step_capture``): its handle, for
    ``cain_graph_launch`` / ``cain_graph_destroy``."""
    err = ctypes.c_int(0)
    g = load().cain_step_capture(ctypes.byref(step), int(steps), stream, ctypes.byref(err))
    if not g:
        raise RuntimeError(f"hipGraph capture failed (err={err.value})")
    return g


def _gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("cain_amd.ops kernels need GPU tensors")


# ---------------------------------------------------------------- ops
_ws_cache: dict = {}


def gemm_ws_bytes(n: int, k: int, m: int) -> int:
    """Workspace the batched GEMM path needs for this shape (0: the skinny kernel runs it)."""
    return int(load().cain_gemm_ws_bytes(n, k, m))


def set_wide_gemm_min_m(m: int) -> None:
    """Rows from which GEMMs run on the wide-batch kernel (csrc/wgemm.hip; default 64, 0 disables): A/B switch
    for tests and tuning, read at every launch and graph capture."""
    load().cain_wgemm_set_min_m(int(m))


def wide_gemm_eligible(n: int, k: int, m: int) -> bool:
    return bool(load().cain_wgemm_eligible(n, k, m))


def set_wide_gemm_plan(n: int, k: int, bm: int, ks: int, variant: int = -1) -> None:
    """Per-shape wide-GEMM plan (csrc/wgemm.hip): split count ``ks`` (<= 0: the default rule) and ring
    ``variant`` (< 0: the global one) for N = n, K = k with the bm-row tile (128 or 256)."""
    if load().cain_wgemm_set_shape(int(n), int(k), int(bm), int(ks), int(variant)) != 0:
        raise RuntimeError("wide-GEMM plan table full")


def set_wide_gemm_variant(v: int) -> None:
    """Global wide-GEMM ring variant (csrc/wgemm.hip; per-shape plans override it): 0 default, 4 fp32 slabs;
    7 / 8 / 9 the timestamped / DMA-only / MFMA-only diagnostic builds of tools/wgemm_trace.py / wgemm_bench.py."""
    load().cain_wgemm_set_variant(int(v))


def set_wide_gemm_inline(mode: int) -> None:
    """Split-K combine of the wide GEMM (csrc/wgemm.hip wg_inline_combine): 0 a separate wgemm_reduce_kernel launch (default),
    1 inside the GEMM launch (A/B runs), 2 inside the launch with partners that never wait (tests)."""
    load().cain_wgemm_set_inline(int(mode))


def wide_gemm_inline_mode() -> int:
    return int(load().cain_wgemm_get_inline())


def wide_gemm_inline(n: int, k: int, m: int) -> bool:
    """Whether the next wide-GEMM launch of this shape combines its split-K slabs in-launch."""
    return bool(load().cain_wgemm_inline(int(n), int(k), int(m)))


def clear_wide_gemm_plans() -> None:
    load().cain_wgemm_clear_shapes()


def wide_gemm_plan(n: int, k: int, m: int) -> Optional[tuple]:
    """(split count, ring variant) the next wide-GEMM launch of this shape uses; None if not eligible."""
    v = int(load().cain_wgemm_plan(n, k, m))
    return None if v < 0 else (v // 64, v % 64)


def _workspace(device, nbytes: int) -> Optional[torch.Tensor]:
    """Per-device zero-initialised GEMM workspace, grown on demand (its counters self-reset)."""
    if nbytes <= 0:
        return None
    key = torch.device(device)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.zeros(nbytes // 4 + 1, device=key, dtype=torch.int32)
        _ws_cache[key] = ws
    return ws


def _gemm_record(w, sc, x, n: int, epi: int, bias, out, norm: bool, eps: float, rope, n_out: Optional[int] = None):
    """The call record of y[M, n_out] = epi(x @ w^T) and ``out``: checked (``EPI_RESID`` updates it in place) or
    allocated; ``rope``: the ``EPI_QKV_ROPE`` arguments, an 8-bit cache (``is_fp8_cache``) sets ``EPI_KV_FP8``."""
    M, K = x.shape
    if n_out is None:
        n_out = n // 2 if epi in (EPI_SILU, EPI_GELU) else n
    if epi == EPI_RESID:
        assert out is not None and out.shape == (M, n_out), "EPI_RESID updates `out` (the residual) in place"
    if epi == EPI_QKV_ROPE:
        assert rope is not None, "EPI_QKV_ROPE needs the rope/cache arguments"
    if out is None:
        out = torch.empty(M, n_out, device=x.device, dtype=torch.float32 if epi == EPI_F32 else torch.bfloat16)
    r = rope or {}
    if rope and is_fp8_cache(r["kc"]):
        epi |= EPI_KV_FP8
    g = CainGemm(W=_p(w), sc=_p(sc), X=_p(x), ldx=x.stride(0), K=K, N=n, M=M, Y=_p(out), ldy=out.stride(0),
                 bias=_p(bias), norm=int(bool(norm)), eps=eps, slot=_p(r.get("slot")), pos=_p(r.get("pos")),
                 cos_t=_p(r.get("cos_t")), sin_t=_p(r.get("sin_t")), kc=_p(r.get("kc")),
                 vtc=_p(r.get("vtc")), H=r.get("H", 0), Hkv=r.get("Hkv", 0), hd=r.get("hd", 0),
                 T_max=r["kc"].shape[-2] if rope else 0, epi=epi)
    return g, out


def _gemm_bf16(g: CainGemm, device, waves: int, batched: bool) -> int:
    g.waves = waves
    g.ws_bytes = gemm_ws_bytes(g.N, g.K, g.M) if batched else 0
    ws = _workspace(device, g.ws_bytes)
    g.ws = _p(ws)
    return load().cain_gemm_bf16(g, _stream())


def skinny_gemm(wp: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16, bias=None,
                out: Optional[torch.Tensor] = None, waves: int = 0, norm: bool = False, eps: float = 1e-6,
                batched: bool = True) -> torch.Tensor:
    """y[M, n] = epi(B(x)[M, K] @ W^T) with W packed by ``pack_mfma_a`` (gate/up interleaved for act epis).

    ``norm``: fused RMSNorm of x, y = rsqrt(mean(x^2) + eps) * (x @ W^T) where the norm gain must already
    be folded into W (``models.weights.fold_gain``).
    ``EPI_RESID``: ``out`` is the residual stream, updated in place.
    ``batched``: 16 < M <= 64 runs the LDS-staged split-K kernel (False forces the skinny kernel).
    """
    _gpu(wp, x)
    M, K = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    assert wp.shape[1] * 32 == K and wp.shape[0] * 16 == n, (tuple(wp.shape), K, n)
    g, out = _gemm_record(wp, None, x, n, epi, bias, out, norm, eps, None)
    _check(_gemm_bf16(g, x.device, waves, batched), "skinny_gemm")
    return out


def is_fp8_cache(t: torch.Tensor) -> bool:
    """An fp8 (e4m3) KV cache: uint8 storage (the engine's) or torch.float8_e4m3fn."""
    return t.dtype in (torch.uint8, torch.float8_e4m3fn)


def qkv_rope(wp, x, n, q_out, kc, vtc, slot, pos, cos_t, sin_t, H, Hkv, hd, bias=None, norm: bool = False,
             eps: float = 1e-6, waves: int = 0, batched: bool = True) -> None:
    """Fused QKV projection (+RMSNorm, +bias) -> RoPE -> Q buffer / K cache / V^T cache.  8-bit caches
    (``is_fp8_cache``) receive e4m3 elements (EPI_KV_FP8)."""
    rope = dict(kc=kc, vtc=vtc, slot=slot, pos=pos, cos_t=cos_t, sin_t=sin_t, H=H, Hkv=Hkv, hd=hd)
    g, _ = _gemm_record(wp, None, x, n, EPI_QKV_ROPE, bias, q_out, norm, eps, rope)
    _check(_gemm_bf16(g, x.device, waves, batched), "qkv_rope")


def gemm_w8(wq: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16, bias=None,
            out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-6, rope=None,
            cmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp8-weight GEMM (``csrc/gemm_w8.hip``, M <= 64): y = epi(B(x) @ (q * scale)^T) with q packed by
    ``models.weights.pack_mfma_a_fp8`` and ``scale`` the per-row fp32 scales.  Same epilogues and RMSNorm
    fusion as ``skinny_gemm``; ``rope`` = dict(kc, vtc, slot, pos, cos_t, sin_t, H, Hkv, hd) for
    ``EPI_QKV_ROPE`` (``out`` is then the Q buffer)."""
    lib = load()
    _gpu(wq, scale, x)
    M, K = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and 1 <= M <= 64
    assert wq.dtype == torch.uint8 and wq.shape[0] * 16 == n and wq.shape[1] * 64 == K, (tuple(wq.shape), K, n)
    assert scale.dtype == torch.float32 and scale.numel() == n
    g, out = _gemm_record(wq, scale, x, n, epi, bias, out, norm, eps, rope)
    _cmax_set(lib, cmax, g.epi)
    _check(lib.cain_gemm_fp8(g, _stream()), "gemm_w8")
    _cmax_check(lib, cmax)
    return out


def gemm_w4(wq: torch.Tensor, wsc: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16, bias=None,
            out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-6, rope=None,
            cmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MXFP4-weight GEMM (``csrc/gemm_w4.hip``, M <= 64): y = epi(B(x) @ dequant(codes, scales)^T) with
    (``wq``, ``wsc``) = ``models.weights.pack_mxfp4(...)``.  Same epilogues, RMSNorm fusion and ``rope`` arguments
    as ``gemm_w8``."""
    lib = load()
    _gpu(wq, wsc, x)
    M, K = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and 1 <= M <= 64
    assert wq.dtype == torch.uint8 and wq.shape[0] * 16 == n and wq.shape[1] * 128 == K, (tuple(wq.shape), K, n)
    assert wsc.dtype == torch.uint8 and wsc.numel() * 32 == n * K
    g, out = _gemm_record(wq, wsc, x, n, epi, bias, out, norm, eps, rope)
    g.ws_bytes = int(lib.cain_gemm_w4_ws_bytes(n, K, M))
    ws = _w4_ws(x.device, g.ws_bytes)
    g.ws = _p(ws)
    _cmax_set(lib, cmax, g.epi)
    _check(lib.cain_gemm_mxfp4(g, _stream()), "gemm_w4")
    _cmax_check(lib, cmax)
    return out


_W4_WS: dict = {}


def _cmax_set(lib, cmax, epi: int) -> None:
    """``cmax`` ([M][N / 16] fp32): the few-row fp32-logits GEMM also writes each row's 16-column chunk maxima (the
    chunk-maximum samplers' input, gemm_epi.h epi_cmax)."""
    if cmax is not None:
        assert epi == EPI_F32 and cmax.dtype == torch.float32 and cmax.is_contiguous()
        lib.cain_gemm_set_cmax(_p(cmax))


def _cmax_check(lib, cmax) -> None:
    if cmax is not None and int(lib.cain_gemm_cmax_take()) != 1:
        raise RuntimeError("this GEMM shape does not write chunk maxima (few-row stream kernels only)")


def _gemm_q(fmt: int, wq, sbuf, x, n: int, epi: int, bias, out, norm: bool, eps: float, rope, gain: bool, cmax,
            tile0: int, name: str) -> torch.Tensor:
    """``gemm_q4`` / ``gemm_q6``: the argument checks and the call (``fmt`` 0 Q4_0, 1 Q4_K, 2 Q6_K; ``tile0``: Q6_K)."""
    lib = load()
    _gpu(wq, sbuf, x)
    M, K = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and M >= 1
    assert wq.dtype == torch.uint8 and wq.shape[0] * 16 == n and wq.shape[1] * 128 == K, (tuple(wq.shape), K, n)
    sc_bytes, dd_bytes = n * K // 16, (n * K // 64 if fmt != 0 else 0)
    assert sbuf.dtype == torch.uint8 and sbuf.numel() == sc_bytes + dd_bytes + (4 * K if gain else 0)
    if fmt == 2:
        assert epi in (EPI_BF16, EPI_RESID, EPI_F32, EPI_QKV_ROPE), "gemm_q6 has no gate/up activation epilogue"
    n_out = n // 2 if epi in (EPI_SILU, EPI_GELU) else 16 * tile0 + n
    if epi == EPI_QKV_ROPE and fmt == 2:
        assert rope is not None and out is not None, "EPI_QKV_ROPE needs the rope/cache arguments and the q rows"
    elif out is not None and fmt == 2:
        assert out.shape[1] >= n_out
    assert fmt != 2 or bias is None or bias.numel() >= n_out
    g, out = _gemm_record(wq, sbuf, x, n, epi, bias, out, norm, eps, rope, n_out)
    g.fmt, g.tile0, g.dd = int(fmt), int(tile0), sbuf.data_ptr() + sc_bytes
    if gain:
        g.gain = sbuf.data_ptr() + sc_bytes + dd_bytes
    _cmax_set(lib, cmax, g.epi)
    _check(lib.cain_gemm_gguf(g, _stream()), name)
    _cmax_check(lib, cmax)
    return out


def gemm_q4(fmt: int, wq: torch.Tensor, sbuf: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16,
            bias=None, out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-6, rope=None,
            gain: bool = False, cmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GGUF Q4_0 (``fmt`` 0) / Q4_K (1) weight GEMM (``csrc/gemm_qstream.hip``; any M: rows beyond the stream kernel's
    LDS copy run on ``csrc/gemm_qtile.hip``, one pass over the weights per 64 rows, see ``set_q_tile``): y = epi(B(x) @
    W^T) with W the blocks' exact values and (``wq``, ``sbuf``) = ``models.q4.pack_q4(...)``; ``gain``: the scale
    buffer ends with the fp32 RMSNorm gain, applied to the activations (``norm`` must be set).  Same epilogues,
    RMSNorm fusion and ``rope`` arguments as ``gemm_w8``."""
    assert fmt in (0, 1), fmt
    return _gemm_q(fmt, wq, sbuf, x, n, epi, bias, out, norm, eps, rope, gain, cmax, 0, "gemm_q4")


def gemm_q6(wq: torch.Tensor, sbuf: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16, bias=None,
            out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-6, rope=None, gain: bool = False,
            cmax: Optional[torch.Tensor] = None, tile0: int = 0) -> torch.Tensor:
    """GGUF Q6_K weight GEMM (``csrc/gemm_qstream.hip``; any M: rows beyond the stream kernel's LDS copy run on
    ``csrc/gemm_qtile.hip``, one pass over the weights per 64 rows, see ``set_q_tile``): y = epi(B(x) @ W^T) with
    W the blocks' exact values and (``wq``, ``sbuf``) = ``models.q4.pack_q6(...)``.  Epilogues EPI_BF16 / EPI_RESID
    / EPI_F32 / EPI_QKV_ROPE; ``gain``, ``norm``, ``rope`` and ``cmax`` as ``gemm_q4``.  ``tile0``: the 16-row tile
    the first of the ``n`` weight rows is in the epilogue's eyes -- output columns (``out`` then has at least 16
    tile0 + n), ``bias`` (indexed from row 0 of the whole projection) and, under EPI_QKV_ROPE, the head or V row:
    the V rows of a fused QKV projection run as a launch of their own with ``tile0 = (H + Hkv) hd / 16``."""
    return _gemm_q(2, wq, sbuf, x, n, epi, bias, out, norm, eps, rope, gain, cmax, tile0, "gemm_q6")


def set_q_tile(mode: int) -> None:
    """Path of the GGUF GEMMs (``gemm_q4`` / ``gemm_q6`` and the runtime's): -1 the rule (the many-row tile kernels of
    ``csrc/gemm_qtile.hip`` where they measured faster than the few-row stream kernels: from 17 rows, and from 8 rows
    where the stream kernels need 4 or more passes; profiles/r8/q_tile/README.md), 0 never the tile kernels (M rows as
    ceil(M / rows) stream launches), 1 always (also M = 1).  Read at every launch and graph capture.  Tests / tuning."""
    load().cain_gemm_q_set_tile(int(mode))


def set_q_tile_nb(nb: int) -> None:
    """Row blocks per wave of the Q4 tile kernels (1 or 2; 0: the rule, gemm_qtile.hip q_tile_nb; Q6_K has 1 only).
    Tests reach both instances at small N with it; tuning."""
    load().cain_gemm_q_set_tile_nb(int(nb))


def gemm_q_passes(fmt: int, k: int, m: int, epi: int = EPI_BF16) -> int:
    """How many times a GGUF GEMM of ``m`` rows streams its weight matrix under the current ``set_q_tile`` mode
    (``fmt`` 0 Q4_0, 1 Q4_K, 2 Q6_K); -1 where the entry refuses the shape (K too long for the stream rows)."""
    return int(load().cain_gemm_q_passes(int(fmt), int(k), int(m), int(epi)))


def _w4_ws(device, nbytes: int) -> torch.Tensor:
    """Zeroed split-K workspace of the W4 GEMMs (its tickets are left zero by every launch), grown as needed."""
    t = _W4_WS.get(device)
    if t is None or t.numel() < nbytes:
        t = _W4_WS[device] = torch.zeros(max(nbytes, 1 << 16), device=device, dtype=torch.uint8)
    return t


def set_w4_split(ks: int) -> None:
    """Split-K of the few-row MXFP4 stream kernel (csrc/gemm_w4.hip w4_split): 0 = the rule (narrow outputs over
    fewer tiles than CUs get up to 4 k ranges of >= 32 quads), 1 = off, k > 1 = k ranges wherever the shape allows."""
    load().cain_gemm_w4_set_split(int(ks))


def set_w4_split_cap(cap: int) -> None:
    """A/B of the split rule's budget: tiles x k ranges <= ``cap`` x CUs (1: the rule)."""
    load().cain_gemm_w4_set_split_cap(int(cap))


def set_w4_split_min_quads(q: int) -> None:
    """A/B of the split rule's shortest k range, in 128-wide quads (32: the rule)."""
    load().cain_gemm_w4_set_split_min_quads(int(q))


def w4_split(n: int, k: int, m: int, epi: int, ws_bytes: int = 1 << 30) -> int:
    """k ranges the W4 GEMM of this shape runs with (given a workspace of ``ws_bytes``)."""
    return int(load().cain_gemm_w4_split(n, k, m, epi, ws_bytes))


def set_w4_variant(v: int) -> None:
    """Force the few-row MXFP4 kernel shape (gemm_w4.hip W4Var index; -1: the shape rule; a stream shape whose LDS
    copy cannot hold the rows falls back to the rule).  Tests / tuning."""
    load().cain_gemm_w4_set_variant(int(v))


def set_w4_occupancy(wgs_per_cu: int) -> None:
    """Workgroups per CU of the persistent single-stream MXFP4 grid (0: 2 of 8 waves / 4 of 4 waves).  Tuning."""
    load().cain_gemm_w4_set_occupancy(int(wgs_per_cu))


def w4_variant(n: int, k: int, m: int, epi: int = EPI_BF16) -> int:
    """The W4Var index the shape rule picks for an (N, K, M) problem with epilogue ``epi``."""
    return int(load().cain_gemm_w4_variant(int(n), int(k), int(m), int(epi)))


def quant_rows(x: torch.Tensor, norm: bool = False, eps: float = 1e-6, x8: Optional[torch.Tensor] = None):
    """Per-row e4m3 quantisation of bf16 activations (csrc/wgemm8.hip quant_rows_kernel): returns (x8 uint8
    [M, K], xs fp32 [M]) with x ~= e4m3(x8) * amax/448 and xs = amax/448 * (rsqrt(mean(x^2) + eps) if norm).
    ``x8``: the output rows, uint8 [M, K] of any row pitch (a view into a wider buffer, as the runtime's)."""
    lib = load()
    _gpu(x, x8)
    M, K = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    if x8 is None:
        x8 = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    assert x8.dtype == torch.uint8 and x8.shape == (M, K) and x8.stride(1) == 1, (x8.dtype, tuple(x8.shape))
    xs = torch.empty(M, device=x.device, dtype=torch.float32)
    _check(lib.cain_quant_rows(_p(x), x.stride(0), K, M, _p(x8), x8.stride(0), _p(xs), int(bool(norm)), eps,
                               _stream()), "quant_rows")
    return x8, xs


def w8a8_eligible(n: int, k: int, m: int) -> bool:
    return bool(load().cain_w8a8_eligible(n, k, m))


def _gemm_a8(name: str, entry: str, w, sc, x, n: int, epi: int, bias, out, norm: bool, eps: float, rope) -> torch.Tensor:
    """``gemm_w8a8`` / ``gemm_w4a8`` after their weight checks: the rows quantised, the record on them, the call."""
    lib = load()
    M, K = x.shape
    assert w8a8_eligible(n, K, M), (n, K, M)
    g, out = _gemm_record(w, sc, x, n, epi, bias, out, False, 0.0, rope)
    x8, xs = quant_rows(x, norm, eps)
    g.X, g.ldx, g.xs = x8.data_ptr(), K, xs.data_ptr()
    g.ws_bytes = int(lib.cain_w8a8_ws_bytes(n, K, M))
    ws = _workspace(x.device, g.ws_bytes)
    g.ws = _p(ws)
    _check(getattr(lib, entry)(g, _stream()), name)
    return out


def gemm_w8a8(wq8: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16, bias=None,
              out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-6, rope=None) -> torch.Tensor:
    """W8A8 wide GEMM (csrc/wgemm8.hip, 16 < M <= 256): the bf16 rows of ``x`` are quantised per row to e4m3
    (``quant_rows``, the RMSNorm folded into the row scale when ``norm``), then y = epi(xs * scale * x8 . q^T)
    with q packed by ``models.weights.pack_mfma_a_fp8_k128``.  Epilogues and ``rope`` as ``gemm_w8``."""
    _gpu(wq8, scale, x)
    K = x.shape[1]
    assert wq8.dtype == torch.uint8 and wq8.shape[0] * 16 == n and wq8.shape[1] * 64 == K, (tuple(wq8.shape), K, n)
    return _gemm_a8("gemm_w8a8", "cain_gemm_fp8a8", wq8, scale, x, n, epi, bias, out, norm, eps, rope)


def gemm_w4a8(wq: torch.Tensor, wsc: torch.Tensor, x: torch.Tensor, n: int, epi: int = EPI_BF16, bias=None,
              out: Optional[torch.Tensor] = None, norm: bool = False, eps: float = 1e-6, rope=None) -> torch.Tensor:
    """W4A8 wide GEMM (csrc/wgemm8.hip FP4, 16 < M <= 256): MXFP4 weights in the few-row kernel's packing
    (``models.weights.pack_mxfp4``: wq uint8 [N/16, K/128, 64, 16], wsc e8m0 bytes [N/16, K/128, 64]) on the
    block-scaled f8f6f4 MFMA against the per-row e4m3 quantisation of ``x`` (``quant_rows``); y = epi(xs * x8 . W^T).
    Epilogues and ``rope`` as ``gemm_w8a8``."""
    _gpu(wq, wsc, x)
    K = x.shape[1]
    assert wq.dtype == torch.uint8 and tuple(wq.shape) == (n // 16, K // 128, 64, 16), (tuple(wq.shape), K, n)
    assert wsc.dtype == torch.uint8 and wsc.numel() * 32 == n * K, (tuple(wsc.shape), K, n)
    return _gemm_a8("gemm_w4a8", "cain_gemm_mxfp4a8", wq, wsc, x, n, epi, bias, out, norm, eps, rope)


def set_w4a8_min_rows(m: int) -> None:
    """Rows above which an MXFP4 engine's forwards run the W4A8 wide kernel instead of the W4A16 few-row one
    (runtime.hip; default 16, the W4A8 minimum: W4A8 is 1.5-2.7x faster at 24-64 rows,
    profiles/r4/ab/w4a8_crossover.txt).  Read at every forward / graph capture."""
    load().cain_w4a8_set_min_rows(int(m))


def rmsnorm(x: torch.Tensor, g: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = load()
    _gpu(x, g)
    M, d = x.shape
    out = torch.empty_like(x) if out is None else out
    _check(lib.cain_rmsnorm(_p(x), x.stride(0), _p(g), _p(out), out.stride(0), M, d, eps, _stream()), "rmsnorm")
    return out


def embed(tok: torch.Tensor, table: torch.Tensor, scale: float = 1.0, out=None) -> torch.Tensor:
    lib = load()
    M = tok.shape[0]
    d = table.shape[1]
    out = torch.empty(M, d, device=table.device, dtype=table.dtype) if out is None else out
    _check(lib.cain_embed(_p(tok), _p(table), _p(out), out.stride(0), M, d, scale, _stream()), "embed")
    return out


def pool_rows(x: torch.Tensor, gain: Optional[torch.Tensor], eps: float, seg_off: torch.Tensor, seg_dst: torch.Tensor,
              mode: int, acc: torch.Tensor, cnt: torch.Tensor, rinv: torch.Tensor, d: Optional[int] = None) -> int:
    """Embedding pooling of bf16 rows ``x [M, ldx]`` (csrc/pool.hip ``cain_pool_rows``): each run ``seg_off[s] ..
    seg_off[s + 1]`` of rows goes, under RMSNorm with the fp32 ``gain``, into row ``seg_dst[s]`` of the fp32 ``acc
    [B, d]`` and the int32 ``cnt [B]`` (``POOL_MEAN``: added in ascending row order; ``POOL_LAST``: the run's final
    row written); ``rinv [M]`` receives the rows' RMSNorm scales.  Returns the entry's code: 0, or -1 for what it
    refuses before any launch (``d`` not a multiple of 8 or above 16384, a null gain)."""
    _gpu(x, gain, seg_off, seg_dst, acc, cnt, rinv)
    d = x.shape[1] if d is None else d
    return int(load().cain_pool_rows(_p(x), x.stride(0), x.shape[0], d, _p(gain), float(eps), _p(seg_off), _p(seg_dst),
                                     seg_dst.numel(), int(mode), _p(acc), _p(cnt), _p(rinv), _stream()))


def pool_finish(acc: torch.Tensor, cnt: torch.Tensor, out: torch.Tensor, normalize: bool = True) -> int:
    """``out[b] = acc[b] / cnt[b]``, L2-normalised with ``normalize`` (csrc/pool.hip ``cain_pool_finish``); rows with
    ``cnt[b] == 0`` are left untouched."""
    _gpu(acc, cnt, out)
    return int(load().cain_pool_finish(_p(acc), _p(cnt), _p(out), acc.shape[0], acc.shape[1], int(bool(normalize)),
                                       _stream()))


# ---------------------------------------------------------------- KV-cache layout (attention.hip header)
def pack_kcache(k: torch.Tensor) -> torch.Tensor:
    """Natural K ``[..., T, hd]`` -> the fragment-major K cache layout (same shape and element count):
    per 16 positions x 32 head dims one 1-KiB MFMA A fragment, lane = (t & 15) + 16 * ((d & 31) >> 3)."""
    *lead, T, hd = k.shape
    n = len(lead)
    t = k.reshape(*lead, T // 16, 16, hd // 32, 4, 8)                 # [u, r, s, q, e]
    t = t.permute(*range(n), n, n + 2, n + 3, n + 1, n + 4)           # [u, s, q, r, e]
    return t.contiguous().reshape(*lead, T, hd)


def unpack_kcache(p: torch.Tensor) -> torch.Tensor:
    *lead, T, hd = p.shape
    n = len(lead)
    t = p.reshape(*lead, T // 16, hd // 32, 4, 16, 8)                 # [u, s, q, r, e]
    t = t.permute(*range(n), n, n + 3, n + 1, n + 2, n + 4)           # [u, r, s, q, e]
    return t.contiguous().reshape(*lead, T, hd)


def pack_vcache(v: torch.Tensor) -> torch.Tensor:
    """Natural V ``[..., T, hd]`` -> the fragment-major V^T cache layout, returned as ``[..., hd, T]`` (the
    engine's buffer shape): per 16 head dims x 32 positions one 1-KiB PV A fragment in the permuted k order
    of P, lane = (d & 15) + 16 * ((t & 15) >> 2), element 4 * ((t >> 4) & 1) + (t & 3)."""
    *lead, T, hd = v.shape
    n = len(lead)
    t = v.reshape(*lead, T // 32, 2, 4, 4, hd // 16, 16)              # [b, h, hq, j, c, dr]
    t = t.permute(*range(n), n, n + 4, n + 2, n + 5, n + 1, n + 3)    # [b, c, hq, dr, h, j]
    return t.contiguous().reshape(*lead, hd, T)


def unpack_vcache(p: torch.Tensor) -> torch.Tensor:
    """Inverse of ``pack_vcache``: ``[..., hd, T]`` buffer -> natural V ``[..., T, hd]``."""
    *lead, hd, T = p.shape
    n = len(lead)
    t = p.reshape(*lead, T // 32, hd // 16, 4, 16, 2, 4)              # [b, c, hq, dr, h, j]
    t = t.permute(*range(n), n, n + 4, n + 2, n + 5, n + 1, n + 3)    # [b, h, hq, j, c, dr]
    return t.contiguous().reshape(*lead, T, hd)


def kfrag_off(t: int, d: int, hd: int) -> int:
    """Host mirror of common.h kfrag_off (element offset inside one (slot, kv head) block)."""
    return ((t >> 4) * (hd >> 5) + (d >> 5)) * 512 + ((t & 15) + 16 * ((d & 31) >> 3)) * 8 + (d & 7)


def vfrag_off(t: int, d: int, hd: int) -> int:
    """Host mirror of common.h vfrag_off."""
    return ((t >> 5) * (hd >> 4) + (d >> 4)) * 512 + ((d & 15) + 16 * ((t & 15) >> 2)) * 8 + 4 * ((t >> 4) & 1) + (t & 3)


def kv_copy_prefix(kcache: torch.Tensor, vtcache: torch.Tensor, L: int, S: int, Hkv: int, hd: int, T_max: int,
                   pairs, stream=None, kv_layer_elems: Optional[int] = None) -> int:
    """Copy cache positions ``[0, n)`` of slot ``src`` to slot ``dst`` for every ``(src, dst, n)`` of ``pairs``: all
    layers, both caches, every kv head, one launch (csrc/kv_prefix.hip) on ``stream`` (a torch stream; default the
    current one).  Returns the entry's code: 0, or -1 when it refused the arguments (nothing launched, the caches
    untouched) -- callers that cannot go on without the copy raise on it."""
    lib = load()
    _gpu(kcache, vtcache)
    kv8 = is_fp8_cache(kcache)
    assert kv8 == is_fp8_cache(vtcache)
    pairs = [tuple(int(x) for x in p) for p in pairs]
    n = len(pairs)
    arr = lambda k: (ci * max(n, 1))(*[p[k] for p in pairs])  # noqa: E731
    elems = int(kv_layer_elems) if kv_layer_elems is not None else S * Hkv * T_max * hd
    st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    return int(lib.cain_kv_copy_prefix(_p(kcache), _p(vtcache), elems, L, S, Hkv, hd, T_max, int(kv8),
                                       arr(0), arr(1), arr(2), n, st))


def kv_copy_prefix_ref(kcache: torch.Tensor, vtcache: torch.Tensor, L: int, S: int, Hkv: int, hd: int, T_max: int,
                       pairs) -> None:
    """The same copy on CPU tensors, in place, from the definition: both caches unpacked to natural
    ``[layer, slot, kv head, position, head dim]``, positions ``< n`` of ``dst`` assigned from ``src`` one by one,
    and packed again (no byte ranges, no offset arithmetic of the kernel's)."""
    k = unpack_kcache(kcache.view(L, S, Hkv, T_max, hd)).clone()
    v = unpack_vcache(vtcache.view(L, S, Hkv, hd, T_max)).clone()
    k0, v0 = k.clone(), v.clone()  # every pair reads the caches as they were
    for src, dst, n in pairs:
        for t in range(int(n)):
            k[:, dst, :, t] = k0[:, src, :, t]
            v[:, dst, :, t] = v0[:, src, :, t]
    kcache.copy_(pack_kcache(k).reshape(kcache.shape))
    vtcache.copy_(pack_vcache(v).reshape(vtcache.shape))


def attention_ml_floats(M: int, H: int, Hkv: int, nsplit: int) -> int:
    """Size of the (max, sum) partial workspace: one 128-B-aligned region per (row, kv head)."""
    G = H // Hkv
    return M * Hkv * ((G * nsplit * 2 + 31) // 32) * 32


def attention(q, kc, vtc, slot, pos, H, Hkv, hd, nsplit, scale, out=None, part_o=None, part_ml=None,
              counters=None, kscale: float = 1.0, vscale: float = 1.0):
    """Decode attention over the fragment-major caches (csrc/attention.hip); 8-bit caches (``is_fp8_cache``)
    hold e4m3 elements whose values are element * kscale / vscale."""
    lib = load()
    M = q.shape[0]
    T_max = kc.shape[-2]
    if part_o is None:
        part_o = torch.empty(M * H * nsplit * hd, device=q.device, dtype=torch.float32)
        part_ml = torch.empty(attention_ml_floats(M, H, Hkv, nsplit), device=q.device, dtype=torch.float32)
    if counters is None:
        counters = torch.zeros(M * Hkv, device=q.device, dtype=torch.int32)
    out = torch.empty(M, H * hd, device=q.device, dtype=torch.bfloat16) if out is None else out
    kv8 = is_fp8_cache(kc)
    assert kv8 == is_fp8_cache(vtc)
    _check(lib.cain_attention_ex(_p(q), _p(kc), _p(vtc), _p(slot), _p(pos), _p(part_o), _p(part_ml), _p(counters),
                                 _p(out), out.stride(0), M, H, Hkv, hd, T_max, nsplit, scale, int(kv8), kscale,
                                 vscale, _stream()),
           "attention")
    return out


def set_sample_cm(mode: int) -> None:
    """Chunk-maximum sampler (the LM head writes 16-column chunk maxima, the sampler reads only the chunks above a
    provable threshold; same tokens).  mode 0 off, 1 the round-3 chunk-maximum kernel on every decode forward, 2
    that kernel on forwards of more than 64 rows (42 vs 62 us at 256 rows; the two-stage kernel below), 3 the lean
    chunk-maximum kernel (sample.hip sample_lean_kernel) on every forward whose LM head wrote the maxima (the
    default: 10.3 vs 30.0 us in-graph at batch 1, profiles/r6/sampler/).  A/B switch for tests and profiles, read at
    every forward / graph capture (env CAIN_SAMPLE_CM at load)."""
    load().cain_sample_set_cm(int(mode))


def set_skinny_split(mode: int) -> None:
    """Split-K rule of the few-row (<= 16) skinny GEMM (gemm.hip skinny_split): 0 never, 1 narrow long-K grids
    (default).  Takes effect at the next launch; an
    engine's workspace is sized at construction, so switch before building one."""
    load().cain_gemm_set_skinny_split(int(mode))


def cu_mask(n_cu: int, total: int = 256) -> list:
    """The 32-bit words of the CU mask a CU-limited stream uses (runtime.hip cain_cu_mask): n_cu of ``total`` CUs
    as evenly spaced whole groups of 8 consecutive bits (balanced over the XCDs under either CU numbering)."""
    words = (total + 31) // 32
    arr = (ctypes.c_uint32 * words)()
    if load().cain_cu_mask(int(n_cu), int(total), arr, words) != 0:
        raise ValueError(f"no CU mask of {n_cu} of {total} CUs (multiples of 8 only)")
    return list(arr)


def set_cu_budget(n_cu: int) -> None:
    """CUs the launch sizing of persistent / CU-proportional grids assumes (0: the device's).  The engine sets it
    around every forward and graph capture of a CU-limited engine (``DecodeEngine(cu_limit=...)``)."""
    load().cain_set_cu_budget(int(n_cu))


def cu_budget() -> int:
    return int(load().cain_get_cu_budget())


def sample_cm_mode() -> int:
    """The chunk-maximum sampler mode in effect (see set_sample_cm)."""
    return int(load().cain_sample_cm_enabled())


def set_attention_ring(variant: int) -> None:
    """LDS-DMA ring body of the wide decode attention (csrc/attention.hip attn_ring_kernel; hd 128, bf16 cache,
    one split, 2 to 64 (row, kv head) pairs per CU): 0 off (the register kernel), 1 on (the default).  A/B switch
    for tests and profiles, read at every launch and graph capture."""
    load().cain_attention_set_ring(int(variant))


def set_attention_body(v: int) -> None:
    """Register-kernel body of the decode attention at head_dim <= 128 (csrc/attention.hip attn_decode_kernel;
    head_dim 256 always runs its one-set body): 2 one register set of K / V fragments held to 128 registers (the
    default), 1 one set at 3 waves per SIMD, 0 two sets ping-pong with a clamped prefetch.  A/B switch for tests
    and profiles, read at every launch and graph capture."""
    if int(v) not in (0, 1, 2):
        raise ValueError(f"attention body {v}: 0, 1 or 2")
    load().cain_attention_set_body(int(v))


SAMPLE_DTYPE = [("temperature", "f4"), ("top_p", "f4"), ("repeat_penalty", "f4"), ("top_k", "i4"),
                ("repeat_last_n", "i4"), ("eos_id", "i4"), ("stop", "i4", (3,)), ("seed", "u8")]
SAMPLE_BYTES = 48  # sizeof(SampleParams), csrc/sample.hip (cain_sample_params_size)


def sample_params_tensor(rows, device) -> torch.Tensor:
    """Pack per-row sampling options (list of dicts; ``stop``: up to 3 further stop ids, default none) into the
    kernel's 48-byte struct array."""
    import numpy as np

    arr = np.zeros(len(rows), dtype=np.dtype(SAMPLE_DTYPE, align=True))
    for i, r in enumerate(rows):
        for f in SAMPLE_DTYPE:
            k = f[0]
            if k == "stop":
                st = [int(x) for x in r.get("stop", ())][:3]
                arr[i][k] = st + [-1] * (3 - len(st))
            else:
                arr[i][k] = r[k]
    assert arr.dtype.itemsize == SAMPLE_BYTES
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


SAMPLE_EXT_DTYPE = [("min_p", "f4"), ("presence_penalty", "f4"), ("frequency_penalty", "f4"), ("reserved", "i4")]
SAMPLE_EXT_BYTES = 16  # sizeof(SampleExt), csrc/sample.hip (cain_sample_ext_size)


def sample_ext_tensor(rows, device) -> torch.Tensor:
    """Pack the further per-row sampling options (list of dicts: ``min_p``, ``presence_penalty``,
    ``frequency_penalty``; a missing key is neutral, 0) into the kernels' 16-byte SampleExt array."""
    import numpy as np

    arr = np.zeros(len(rows), dtype=np.dtype(SAMPLE_EXT_DTYPE, align=True))
    for i, r in enumerate(rows):
        for k in ("min_p", "presence_penalty", "frequency_penalty"):
            arr[i][k] = r.get(k, 0.0)
    assert arr.dtype.itemsize == SAMPLE_EXT_BYTES
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def sample(logits, tok, pos, gen, n_gen, max_new, done, hist, slot, params, T_max, split: bool = False,
           cmax=None, lean: bool = False, ext=None) -> None:
    """On-device sampling + decode-state update (csrc/sample.hip).  ``split``: the two-stage kernel (vocabulary
    slices on 16 workgroups per row, last-arriver merge) that decode forwards of <= 64 rows use; ``cmax`` ([M][V/16]
    fp32 maxima of the logits' 16-column chunks, as the few-row LM head writes them): the chunk-maximum kernel that
    single-stream decode uses (``lean``: the lean chunk-maximum kernel); otherwise the one-workgroup-per-row
    kernel.  ``ext``: the rows' SampleExt records (``sample_ext_tensor``); None is neutral."""
    lib = load()
    M, V = logits.shape[0], logits.shape[1]
    if cmax is not None and lean:
        _check(lib.cain_sample_lean(_p(logits), logits.stride(0), V, _p(cmax), _p(tok), _p(pos), _p(gen),
                                    gen.stride(0), _p(n_gen), _p(max_new), _p(done), _p(hist), _p(slot), T_max, M,
                                    _p(params), _p(ext), _stream()), "sample_lean")
        return
    if cmax is not None:
        _check(lib.cain_sample_cm(_p(logits), logits.stride(0), V, _p(cmax), _p(tok), _p(pos), _p(gen), gen.stride(0),
                                  _p(n_gen), _p(max_new), _p(done), _p(hist), _p(slot), T_max, M, _p(params),
                                  _p(ext), _stream()), "sample_cm")
        return
    if split:
        nb = int(lib.cain_sample_ws_bytes(M))
        ws = _sample_ws(logits.device, nb)
        _check(lib.cain_sample_ex(_p(logits), logits.stride(0), V, _p(tok), _p(pos), _p(gen), gen.stride(0),
                                  _p(n_gen), _p(max_new), _p(done), _p(hist), _p(slot), T_max, M, _p(params), _p(ext),
                                  _p(ws), nb, _stream()), "sample")
        return
    _check(lib.cain_sample(_p(logits), logits.stride(0), V, _p(tok), _p(pos), _p(gen), gen.stride(0), _p(n_gen),
                           _p(max_new), _p(done), _p(hist), _p(slot), T_max, M, _p(params), _p(ext), _stream()),
           "sample")


LOGPROB_TOP_MAX = 20  # top_logprobs limit: entries per token in the top-n buffers (csrc/logprob.hip LP_TOP)


def _lp_nmax(topn: torch.Tensor, nmax: Optional[int]) -> int:
    return int(nmax) if nmax is not None else max(0, int(topn.max()))


def logprob_rows(logits: torch.Tensor, V: int, topn: torch.Tensor, slot=None, done=None, target=None, lse=None,
                 lp=None, top_id=None, top_lp=None, nmax: Optional[int] = None) -> int:
    """Log-softmax statistics of fp32 logits rows ``[M, ldl]`` (``ldl = logits.stride(0) >= V``; csrc/logprob.hip):
    per row m with ``topn[m] >= 0`` (and ``slot[m] >= 0``, ``done[m] == 0`` where given) the log-sum-exp into
    ``lse[m]``, the natural-log softmax of ``target[m]`` into ``lp[m]`` and the ``topn[m]`` most likely ids (logit
    descending, index ascending on ties) with their logprobs into ``top_id / top_lp[m, :topn[m]]`` (``[M, 20]``).
    Other rows are left as they are.  ``nmax``: the largest ``topn`` (default: read from the device).  Returns the
    entry's code: 0, or non-zero when it refused the arguments (``V % 4``, ``ldl < V``, ``nmax > 20``) with nothing
    launched."""
    lib = load()
    _gpu(logits, topn)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and topn.dtype == torch.int32
    for t in (top_id, top_lp):
        assert t is None or (t.is_contiguous() and t.shape[-1] == LOGPROB_TOP_MAX)
    return int(lib.cain_logprob_rows(_p(logits), logits.stride(0), int(V), logits.shape[0], _p(slot), _p(done),
                                     _p(topn), _lp_nmax(topn, nmax), _p(target), _p(lse), _p(lp), _p(top_id),
                                     _p(top_lp), _stream()))


def logprob_keep(M: int, device) -> torch.Tensor:
    """Scratch that ``logprob_pre`` hands to ``logprob_chosen`` for M rows."""
    return torch.zeros(int(load().cain_logprob_keep_bytes(int(M))), device=device, dtype=torch.uint8)


def logprob_pre(logits: torch.Tensor, V: int, topn: torch.Tensor, n_gen, hist, gen: torch.Tensor, top_id, top_lp,
                keep, slot=None, done=None, nmax: Optional[int] = None) -> int:
    """The decode step's statistics, BEFORE the sampler (which may apply the repeat penalty in place on ``logits``):
    the top-n of each wanted live row into the rings at the index of the token about to be generated,
    ``top_id / top_lp[m, n_gen[m], :topn[m]]`` (``[M, ldg, 20]``, ``ldg = gen.stride(0)``), and into ``keep``
    (``logprob_keep``) the row's log-sum-exp, ``n_gen`` and the raw logits of its history ids."""
    lib = load()
    _gpu(logits, topn, keep)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and topn.dtype == torch.int32
    assert top_id.is_contiguous() and top_lp.is_contiguous() and top_id.shape[-1] == LOGPROB_TOP_MAX
    assert keep.numel() >= int(lib.cain_logprob_keep_bytes(logits.shape[0]))
    return int(lib.cain_logprob_pre(_p(logits), logits.stride(0), int(V), logits.shape[0], _p(slot), _p(done),
                                    _p(topn), _lp_nmax(topn, nmax), _p(n_gen), _p(hist), gen.stride(0), _p(top_id),
                                    _p(top_lp), _p(keep), _stream()))


def logprob_chosen(logits: torch.Tensor, V: int, gen: torch.Tensor, keep, lp: torch.Tensor) -> int:
    """AFTER the sampler: ``lp[m, n]`` = the logprob of the token the sampler wrote at ``gen[m, n]`` (n: the row's
    ``n_gen`` before the step), from the raw logit ``logprob_pre`` kept when the id is one of the history ids."""
    lib = load()
    _gpu(logits, gen, keep, lp)
    assert lp.stride(0) == gen.stride(0) and lp.dtype == torch.float32
    return int(lib.cain_logprob_chosen(_p(logits), logits.stride(0), int(V), logits.shape[0], _p(gen), gen.stride(0),
                                       _p(keep), _p(lp), _stream()))


# ------------------------------------------------------------ JSON mode (csrc/grammar.hip, csrc/json_pda.h)
JSON_STATE_BYTES = 16  # sizeof(JsonState): control word, depth word, 64-bit bracket-kind stack
JSON_VOCAB_MAX = 1 << 23  # a masked logit carries its token id in the mantissa


def json_table(pieces, device) -> dict:
    """The vocabulary of JSON mode on the device: ``pieces[t]`` is the bytes token ``t`` appends (empty: a special
    token, never allowed).  Returns ``dict(V, piece_off [V + 1] int32, piece_bytes uint8)``."""
    from ..engine.jsonmode import piece_table

    if len(pieces) > JSON_VOCAB_MAX:
        raise ValueError(f"JSON mode supports vocabularies up to {JSON_VOCAB_MAX} tokens, got {len(pieces)}")
    off, flat = piece_table(pieces)
    return dict(V=len(pieces), piece_off=torch.from_numpy(off).to(device), piece_bytes=torch.from_numpy(flat).to(device))


def json_states(states, device) -> torch.Tensor:
    """``[(ctrl, depth, stack)]`` (engine/jsonmode.py states) as the device's ``[M, 4]`` int32 JsonState rows."""
    import numpy as np

    a = np.zeros((len(states), 2), dtype=np.uint64)
    for i, (c, d, st) in enumerate(states):
        a[i, 0] = (int(d) << 32) | int(c)
        a[i, 1] = int(st)
    return torch.from_numpy(a.view(np.int32).reshape(len(states), 4).copy()).to(device)


def json_states_host(gstate: torch.Tensor) -> list:
    """The inverse of ``json_states``."""
    import numpy as np

    a = np.ascontiguousarray(gstate.detach().cpu().numpy()).view(np.uint64).reshape(-1, 2)
    return [(int(x) & 0xFFFFFFFF, int(x) >> 32, int(y)) for x, y in a]


def json_mask(logits: torch.Tensor, V: int, gram_on, done, gstate, table: dict, cmax=None) -> int:
    """BEFORE the sampler: in every row m of fp32 ``logits [M, ldl]`` with ``gram_on[m] != 0`` and ``done[m] == 0``,
    each token whose bytes cannot continue the row's JSON document from ``gstate[m]`` gets the logit
    ``-(2^100 (1 + t / 2^23))``; accepted tokens and other rows are not written.  ``cmax [M, V / 16]``: the rows'
    16-column chunk maxima, rewritten from the masked logits.  Returns the entry's code (non-zero: refused)."""
    lib = load()
    _gpu(logits, gram_on, done, gstate, table["piece_off"], table["piece_bytes"], cmax)
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and gstate.is_contiguous()
    assert gram_on.dtype == torch.int32 and done.dtype == torch.int32 and int(V) <= table["V"]
    assert cmax is None or (cmax.dtype == torch.float32 and cmax.is_contiguous() and cmax.shape[1] * 16 == int(V))
    return int(lib.cain_json_mask(_p(logits), logits.stride(0), int(V), logits.shape[0], _p(gram_on), _p(done),
                                  _p(gstate), _p(table["piece_off"]), _p(table["piece_bytes"]), _p(cmax), _stream()))


def json_advance(gram_on, gen: torch.Tensor, n_gen, done, gstate, table: dict) -> int:
    """AFTER the sampler: every JSON-mode row that generated a token this step consumes it (``gen[m, n_gen[m] - 1]``);
    a closed top-level object sets ``done[m]``, an invalid token is taken back (``n_gen[m] -= 1``), fails the state
    and sets ``done[m]``."""
    lib = load()
    _gpu(gram_on, gen, n_gen, done, gstate)
    assert gen.dtype == torch.int32 and gen.stride(1) == 1 and gstate.is_contiguous()
    return int(lib.cain_json_advance(gen.shape[0], int(table["V"]), _p(gram_on), _p(gen), gen.stride(0), _p(n_gen),
                                     _p(done), _p(gstate), _p(table["piece_off"]), _p(table["piece_bytes"]),
                                     _stream()))


# ------------------------------------------------------------ stop sequences (csrc/stopseq.hip, csrc/stop_match.h)
STOP_STATE_BYTES = 48  # sizeof(StopState): 32 tail bytes, tokens, bytes, hit_start, hit_which
STOP_MAX = 8
STOP_LEN_MAX = 32


def stop_table_host(rows_of_strings):
    """``(stop_on [M] int32, stop_len [M, 8] int32, stop_bytes [M, 8, 32] uint8)`` CPU tensors of per-row stop
    strings (``str`` or ``bytes``; validated by ``engine.stopseq.parse_stop`` upstream: at most 8 of 1 .. 32 bytes)."""
    import numpy as np

    from ..engine.stopseq import stop_bytes

    M = len(rows_of_strings)
    on, ln = np.zeros(M, dtype=np.int32), np.zeros((M, STOP_MAX), dtype=np.int32)
    by = np.zeros((M, STOP_MAX, STOP_LEN_MAX), dtype=np.uint8)
    for i, row in enumerate(rows_of_strings):
        bs = stop_bytes(row or ())
        if len(bs) > STOP_MAX or any(not 1 <= len(b) <= STOP_LEN_MAX for b in bs):
            raise ValueError(f"row {i}: at most {STOP_MAX} stop strings of 1..{STOP_LEN_MAX} bytes")
        on[i] = int(bool(bs))
        for k, b in enumerate(bs):
            ln[i, k] = len(b)
            by[i, k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(on), torch.from_numpy(ln), torch.from_numpy(by)


def stop_table(rows_of_strings, device):
    """``stop_table_host`` on ``device``: ``(stop_on, stop_len, stop_bytes)``."""
    return tuple(t.to(device) for t in stop_table_host(rows_of_strings))


def stop_states(states, device) -> torch.Tensor:
    """``engine.stopseq`` states as the device's ``[M, 48]`` uint8 StopState rows."""
    import numpy as np

    from ..engine.stopseq import state_bytes

    a = np.frombuffer(b"".join(state_bytes(s) for s in states), dtype=np.uint8).reshape(len(states), STOP_STATE_BYTES)
    return torch.from_numpy(a.copy()).to(device)


def stop_states_host(sstate: torch.Tensor) -> list:
    """The inverse of ``stop_states``."""
    from ..engine.stopseq import state_from_bytes

    a = sstate.detach().cpu().contiguous().view(torch.uint8).reshape(-1, STOP_STATE_BYTES).numpy()
    return [state_from_bytes(r.tobytes()) for r in a]


def stop_advance(stop_on, gen: torch.Tensor, n_gen, done, sstate, stop_len, stop_bytes, table: dict) -> int:
    """AFTER the sampler (and after ``json_advance``): every row with ``stop_on[m] != 0`` that generated a token this
    step (``n_gen[m]`` is one above the tokens its state has consumed) consumes ``gen[m, n_gen[m] - 1]``; a stop string
    that ends inside the token's bytes sets ``done[m]`` and the state's ``hit_start`` / ``hit_which``.  Returns the
    entry's code (non-zero: refused)."""
    lib = load()
    _gpu(stop_on, gen, n_gen, done, sstate, stop_len, stop_bytes, table["piece_off"], table["piece_bytes"])
    assert gen.dtype == torch.int32 and gen.stride(1) == 1 and sstate.is_contiguous()
    assert stop_len.is_contiguous() and stop_bytes.is_contiguous() and stop_len.dtype == torch.int32
    M = gen.shape[0]
    assert sstate.numel() * sstate.element_size() >= M * STOP_STATE_BYTES and stop_len.numel() >= M * STOP_MAX
    assert stop_bytes.numel() >= M * STOP_MAX * STOP_LEN_MAX and stop_bytes.dtype == torch.uint8
    assert min(stop_on.numel(), n_gen.numel(), done.numel()) >= M
    return int(lib.cain_stop_advance(M, int(table["V"]), _p(stop_on), _p(gen), gen.stride(0), _p(n_gen), _p(done),
                                     _p(sstate), _p(stop_len), _p(stop_bytes), _p(table["piece_off"]),
                                     _p(table["piece_bytes"]), _stream()))


_SAMPLE_WS: dict = {}


def _sample_ws(device, nbytes: int) -> torch.Tensor:
    """Zeroed sampler workspace per device (its tickets self-reset), grown on demand."""
    t = _SAMPLE_WS.get(device)
    if t is None or t.numel() * 4 < nbytes:
        t = _SAMPLE_WS[device] = torch.zeros((nbytes + 3) // 4, device=device, dtype=torch.int32)
    return t


# ------------------------------------------------------------ speculative decoding (csrc/spec.hip)
SPEC_K_MAX = 7  # csrc/spec.h
ROW_KEYS = ("tok", "pos", "slot", "n_gen", "max_new", "done", "hist")


def spec_alloc(R: int, K: int, slots: int, T_max: int, vocab: int, device) -> dict:
    """Buffers of speculative decoding for up to ``R`` sequences with ``K`` drafts each (csrc/spec.h): the token
    record per cache slot, the given drafts, the expanded row state of the ``R (K + 1)``-row verify forward, the
    step's drafts and the per-sequence counters."""
    if not 1 <= K <= SPEC_K_MAX:
        raise ValueError(f"speculative K must be in 1..{SPEC_K_MAX}, got {K}")
    X = R * (K + 1)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, device=device, dtype=dt)  # noqa: E731
    return dict(K=int(K), vocab=int(vocab), seq=z(slots, T_max), given=torch.full((R, T_max), -1, device=device,
                                                                                 dtype=torch.int32),
                x_tok=z(X), x_pos=z(X), x_slot=torch.full((X,), -1, device=device, dtype=torch.int32), x_n_gen=z(X),
                x_max_new=z(X), x_done=z(X), x_hist=z(X, 64), x_gen=z(X, T_max),
                x_params=z(X * SAMPLE_BYTES, dt=torch.uint8), nd=z(R), draft=torch.full((R, K), -1, device=device,
                                                                                      dtype=torch.int32),
                drafted=z(R), accepted=z(R), n_step=z(R), step_tokens=z(R, T_max))


def spec_struct(spec: dict, mode: int) -> CainSpec:
    """The kernels' view of ``spec_alloc`` buffers; ``mode`` 0: n-gram drafts, 1: the ``given`` drafts."""
    s = CainSpec()
    s.K, s.mode, s.vocab = int(spec["K"]), int(mode), int(spec["vocab"])
    s.slots, s.lds = spec["seq"].shape[0], spec["seq"].stride(0)
    s.ldv, s.ldt, s.ldg = spec["given"].stride(0), spec["step_tokens"].stride(0), spec["x_gen"].stride(0)
    for k in _SPEC_PTRS:
        setattr(s, k, spec[k].data_ptr())
    return s


def spec_draft(rows: dict, params: torch.Tensor, spec: dict, R: int, mode: int, T_max: int) -> None:
    """Draft for sequences ``[0, R)`` of the decode rows (``ROW_KEYS`` tensors) and write the expanded state."""
    lib = load()
    _gpu(params, *[rows[k] for k in ROW_KEYS])
    assert spec["nd"].shape[0] >= R and rows["tok"].shape[0] >= R
    s = spec_struct(spec, mode)
    _check(lib.cain_spec_draft(ctypes.byref(s), R, T_max, *[_p(rows[k]) for k in ROW_KEYS], _p(params), _stream()),
           "spec_draft")


def spec_accept(rows: dict, gen: torch.Tensor, params: torch.Tensor, spec: dict, R: int, T_max: int) -> None:
    """Commit, per sequence, the tokens the sampler left in ``spec["x_tok"]`` that the step's drafts allow."""
    lib = load()
    _gpu(params, gen, *[rows[k] for k in ROW_KEYS])
    s = spec_struct(spec, 0)
    r = rows
    _check(lib.cain_spec_accept(ctypes.byref(s), R, T_max, _p(r["tok"]), _p(r["pos"]), _p(r["slot"]), _p(r["n_gen"]),
                                _p(r["max_new"]), _p(r["done"]), _p(r["hist"]), _p(gen), gen.stride(0), _p(params),
                                _stream()), "spec_accept")


def _np(t):
    import numpy as np

    return np.array(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)


# ---- draft-model mode (csrc/spec.h CainSpecDraft)
_SPECD_ROWS = ("r_tok", "r_pos", "r_slot", "r_n_gen", "r_max_new", "r_done")


def spec_draft_alloc(spec: dict, dvocab: int, dbos: int) -> dict:
    """Buffers of draft-model mode beside the ``spec_alloc`` buffers ``spec`` (whose record and given drafts they
    share): ``dvalid`` per cache slot, the step's scratch per sequence and the 2 R draft rows."""
    R, T_max, dev = spec["nd"].shape[0], spec["seq"].shape[1], spec["seq"].device
    if not 0 <= int(dbos) < int(dvocab):
        raise ValueError(f"draft bos id {dbos} outside the draft vocabulary ({dvocab})")
    z = lambda *s, dt=torch.int32: torch.zeros(*s, device=dev, dtype=dt)  # noqa: E731
    return dict(K=int(spec["K"]), dvocab=int(dvocab), dbos=int(dbos), seq=spec["seq"], given=spec["given"],
                dvalid=z(spec["seq"].shape[0]), p0=z(R), nd=z(R), r_tok=z(2 * R), r_pos=z(2 * R),
                r_slot=torch.full((2 * R,), -1, device=dev, dtype=torch.int32), r_n_gen=z(2 * R), r_max_new=z(2 * R),
                r_done=z(2 * R), r_hist=z(2 * R, 64), r_gen=z(2 * R, T_max),
                r_params=z(2 * R * SAMPLE_BYTES, dt=torch.uint8))


def spec_draft_struct(sd: dict) -> CainSpecDraft:
    s = CainSpecDraft()
    s.K, s.dvocab, s.dbos = int(sd["K"]), int(sd["dvocab"]), int(sd["dbos"])
    s.slots, s.lds, s.ldv, s.ldg = sd["seq"].shape[0], sd["seq"].stride(0), sd["given"].stride(0), sd["r_gen"].stride(0)
    for k in _SPECD_PTRS:
        setattr(s, k, sd[k].data_ptr())
    return s


def spec_model_rows(rows: dict, params: torch.Tensor, sd: dict, R: int, T_max: int) -> None:
    """The 2 R rows of the first draft forward from sequences ``[0, R)`` of the decode rows."""
    lib = load()
    _gpu(params, *[rows[k] for k in ROW_KEYS])
    assert sd["nd"].shape[0] >= R and rows["tok"].shape[0] >= R
    s = spec_draft_struct(sd)
    _check(lib.cain_spec_model_rows(ctypes.byref(s), R, T_max, *[_p(rows[k]) for k in ROW_KEYS], _p(params),
                                    _stream()), "spec_model_rows")


def spec_model_next(rows: dict, sd: dict, R: int, j: int, T_max: int) -> None:
    """After draft forward ``j``'s sampler: ``d_j`` into ``given``, the rows of forward ``j + 1``."""
    lib = load()
    s = spec_draft_struct(sd)
    _check(lib.cain_spec_model_next(ctypes.byref(s), R, j, T_max, _p(rows["slot"]), _p(rows["n_gen"]), _stream()),
           "spec_model_next")


def spec_dvalid(rows: dict, sd: dict, R: int, T_max: int) -> None:
    """After accept: ``dvalid`` of the sequences' slots from their new positions."""
    lib = load()
    s = spec_draft_struct(sd)
    _check(lib.cain_spec_dvalid(ctypes.byref(s), R, T_max, _p(rows["slot"]), _p(rows["pos"]), _stream()),
           "spec_dvalid")


def spec_model_rows_ref(rows: dict, params, sd: dict, R: int, T_max: int) -> dict:
    """``spec_model_rows`` from the rule (engine/speculative.py), sequence by sequence in Python: numpy arrays of
    everything the kernel writes (the 2 R draft rows, ``p0``, ``nd``, ``given``)."""
    import numpy as np

    from ..engine import speculative as sp

    K = int(sd["K"])
    r = {k: _np(rows[k]) for k in ROW_KEYS}
    hist = r["hist"].reshape(-1, 64)
    par = _np(params).reshape(-1, SAMPLE_BYTES)
    seq, dvalid = _np(sd["seq"]), _np(sd["dvalid"])
    out = {k: np.zeros(2 * R, np.int32) for k in _SPECD_ROWS}
    out.update(r_hist=np.zeros((2 * R, 64), np.int32), r_params=np.zeros((2 * R, SAMPLE_BYTES), np.uint8),
               p0=np.zeros(R, np.int32), nd=np.zeros(R, np.int32), given=_np(sd["given"]))
    for i in range(R):
        sl, pos, ng, mn = int(r["slot"][i]), int(r["pos"][i]), int(r["n_gen"][i]), int(r["max_new"][i])
        live = 0 <= sl < seq.shape[0] and not r["done"][i]
        rec = list(seq[sl, :pos]) + [int(r["tok"][i])] if live else []
        d, catch_up, own = sp.draft_model_rows(rec, pos, ng, K, T_max, mn, int(dvalid[sl]) if live else 0,
                                               int(sd["dvocab"]), int(sd["dbos"]), done=not live, slot=sl)
        out["p0"][i], out["nd"][i] = pos, d
        if live and d < K:
            out["given"][i, ng + d] = -1
        for x, row in ((i, own), (R + i, catch_up)):
            for k, v in zip(_SPECD_ROWS, row):
                out[k][x] = v
            out["r_hist"][x] = hist[i]
            out["r_params"][x] = par[i]
            out["r_params"][x, 20:36] = 0xFF  # eos_id and the three stop ids: -1
    return out


def spec_model_next_ref(rows: dict, sd: dict, R: int, j: int) -> dict:
    """``spec_model_next`` from the rule: numpy copies of rows ``[0, R)`` (with their rings) and ``given`` after it."""
    from ..engine import speculative as sp

    out = {k: _np(sd[k])[:R] for k in _SPECD_ROWS}
    out.update(r_hist=_np(sd["r_hist"])[:R], given=_np(sd["given"]))
    slot, n_gen, p0, nd = _np(rows["slot"]), _np(rows["n_gen"]), _np(sd["p0"]), _np(sd["nd"])
    for i in range(R):
        d, ng = int(nd[i]), int(n_gen[i])
        if d <= 0 or j > d:
            continue
        dj = int(out["r_tok"][i])
        out["given"][i, ng + j - 1] = dj
        out["r_hist"][i, (ng + j - 1) & 63] = dj
        row = sp.draft_model_next(dj, j, int(p0[i]), ng, d, int(slot[i]), int(sd["dvocab"]), int(sd["dbos"]))
        for k, v in zip(_SPECD_ROWS, row):
            out[k][i] = v
    return out


def spec_dvalid_ref(rows: dict, sd: dict, R: int):
    """``spec_dvalid`` from the rule: ``dvalid`` after it."""
    from ..engine import speculative as sp

    out = _np(sd["dvalid"])
    slot, pos, p0, nd = _np(rows["slot"]), _np(rows["pos"]), _np(sd["p0"]), _np(sd["nd"])
    for i in range(R):
        if nd[i] > 0 and 0 <= slot[i] < out.shape[0]:
            out[slot[i]] = sp.dvalid_after(int(p0[i]), int(nd[i]), int(pos[i]))
    return out


def spec_draft_ref(rows: dict, params, spec: dict, R: int, mode: int, T_max: int) -> dict:
    """``spec_draft`` from the rule (engine/speculative.py), sequence by sequence in Python: returns the numpy
    arrays the kernel writes (``x_*`` over the first ``R (K + 1)`` rows, ``nd``, ``draft``)."""
    import numpy as np

    from ..engine import speculative as sp

    K = int(spec["K"])
    K1 = K + 1
    r = {k: _np(rows[k]) for k in ROW_KEYS}
    hist = r["hist"].reshape(-1, 64)
    par = _np(params).reshape(-1, SAMPLE_BYTES)
    seq, given = _np(spec["seq"]), _np(spec["given"])
    out = dict(x_tok=np.zeros(R * K1, np.int32), x_pos=np.zeros(R * K1, np.int32),
               x_slot=np.full(R * K1, -1, np.int32), x_n_gen=np.zeros(R * K1, np.int32),
               x_max_new=np.zeros(R * K1, np.int32), x_done=np.zeros(R * K1, np.int32),
               x_hist=np.zeros((R * K1, 64), np.int32), x_params=np.zeros((R * K1, SAMPLE_BYTES), np.uint8),
               nd=np.zeros(R, np.int32), draft=np.full((R, K), -1, np.int32))
    for i in range(R):
        sl, pos, ng = int(r["slot"][i]), int(r["pos"][i]), int(r["n_gen"][i])
        dr = sp.draft(seq[sl] if 0 <= sl < seq.shape[0] else [], pos, ng, K, T_max, int(r["max_new"][i]),
                      done=bool(r["done"][i]), slot=sl, given=given[i] if mode == 1 else None,
                      vocab=int(spec["vocab"]))
        d = len(dr)
        out["nd"][i] = d
        out["draft"][i, :d] = dr
        for j in range(K1):
            x = i * K1 + j
            out["x_params"][x] = par[i]
            out["x_hist"][x] = sp.draft_ring(hist[i], ng, dr, j) if j <= d else hist[i]
            if j == 0:
                vals = (r["tok"][i], pos, sl, ng, r["max_new"][i], r["done"][i])
            elif j <= d:
                vals = (dr[j - 1], pos + j, sl, ng + j, sp.NO_BUDGET, 0)
            else:
                vals = (0, 0, -1, 0, 0, 0)
            for k, v in zip(("x_tok", "x_pos", "x_slot", "x_n_gen", "x_max_new", "x_done"), vals):
                out[k][x] = v
    return out


def spec_accept_ref(rows: dict, gen, params, spec: dict, R: int, T_max: int) -> dict:
    """``spec_accept`` from the rule, sequence by sequence in Python: returns numpy copies of everything the kernel
    may write (the decode rows, ``gen``, ``seq`` and the counters) after the step."""
    import numpy as np

    from ..engine import speculative as sp

    K = int(spec["K"])
    K1 = K + 1
    out = {k: _np(rows[k]) for k in ROW_KEYS}
    out["hist"] = out["hist"].reshape(-1, 64)
    out["gen"] = _np(gen)
    for k in ("seq", "drafted", "accepted", "n_step", "step_tokens"):
        out[k] = _np(spec[k])
    par = np.ascontiguousarray(_np(params).reshape(-1, SAMPLE_BYTES)).view(np.dtype(SAMPLE_DTYPE, align=True))[:, 0]
    xt, nd, draft = _np(spec["x_tok"]), _np(spec["nd"]), _np(spec["draft"]).reshape(-1, K)
    for i in range(R):
        sl, ng = int(out["slot"][i]), int(out["n_gen"][i])
        if sl < 0 or out["done"][i]:
            continue
        st = sp.SeqState(tok=int(out["tok"][i]), pos=int(out["pos"][i]), max_new=int(out["max_new"][i]),
                         eos_id=int(par[i]["eos_id"]), stop=[int(s) for s in par[i]["stop"]], slot=sl, n_gen=ng,
                         gen=list(out["gen"][i, :ng]), hist=list(out["hist"][i]),
                         seq=list(out["seq"][sl, :int(out["pos"][i]) + 1]))
        d = int(nd[i])
        c = st.commit_step(list(draft[i, :d]), list(xt[i * K1: i * K1 + d + 1]), T_max)
        out["gen"][i, ng: ng + c] = st.gen[ng:]
        out["hist"][i] = st.hist
        out["seq"][sl, : len(st.seq)] = st.seq
        out["tok"][i], out["pos"][i], out["n_gen"][i], out["done"][i] = st.tok, st.pos, st.n_gen, int(st.done)
        out["drafted"][i] += d
        out["accepted"][i] += c - 1
        k = int(out["n_step"][i])
        out["step_tokens"][i, k % out["step_tokens"].shape[1]] = c
        out["n_step"][i] = k + 1
    return out
