"""Engine state checks: the KV cache a ``DecodeEngine`` built, held per (layer, slot, kv head, position) against the
fp32 oracle's K / V of the same tokens, and everything the engine should not have written held bitwise to a sentinel.

The cache is a complete record of what the engine did: one K and one V vector per (layer, slot, kv head, position).
A missing, stale, swapped or misplaced KV write is an error of order 1 (or >= 100 where poison shows) at a named
location, against a rounding floor of order 1e-2; a wrong slot or position handed to a launch is a sentinel that
changed.  ``ALL_CASES`` lists every model / format / length set of ``tests/test_engine_state_gpu.py``; the host checks of
``tests/test_engine_state_cpu.py`` (limits under the cap, sentinel magnitude, planted faults) run over the same list.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from cain_amd import ops
from cain_amd.models import get_config

T_MAX = 256  # max_context of every case
# One fixed finite bit pattern per cache dtype, >= 100 x the largest |K| or |V| of any case (asserted on the host):
# bf16 1.5 * 2^13, e4m3 1.75 * 2^7 (byte 0x76: finite, no NaN encoding).  attention.hip allows any finite value past
# a row's length.
SENTINEL = {"bf16": 12288.0, "fp8": 224.0}
MARGIN = 3.0   # limit = MARGIN x the eager baseline's largest per-vector error in that layer ...
CAP = 0.25     # ... and never more: a wrong vector has error near 1 or above, a poisoned one >= 100
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, eos_id=-1)


# ------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """One model / format / request set.  ``predict[i] == 0``: prompt i only goes through ``last_logits`` (positions
    0 .. L-1 written).  ``a8``: prefill chunks run the W8A8 / W4A8 kernel (activations per row to e4m3) while the
    few-row decode runs A16, so the baseline quantises activations for the prefill positions only."""
    id: str
    model: str
    lengths: Tuple[int, ...]
    predict: Tuple[int, ...]
    weight_dtype: str = "bf16"
    kv_dtype: str = "bf16"
    overrides: Tuple[Tuple[str, int], ...] = ()
    max_batch: int = 4
    a8: bool = False
    seed: int = 17
    # layers whose vectors are compared (None: all); the sentinel check always covers every layer
    compare_layers: Optional[int] = None

    def config(self):
        return dataclasses.replace(get_config(self.model), **dict(self.overrides))

    def tokens_predicted(self) -> Tuple[int, ...]:
        """num_predict after the engine's clamp to the context."""
        return tuple(max(1, min(n, T_MAX - L)) if n else 0 for L, n in zip(self.lengths, self.predict))

    def written(self) -> Tuple[int, ...]:
        """Cache positions each row ends up with (p_last + 1)."""
        return tuple(L + n - 1 if n else L for L, n in zip(self.lengths, self.tokens_predicted()))

    def prompts(self) -> List[List[int]]:
        return [prompt_ids(L, self.config().vocab, self.seed + 31 * i) for i, L in enumerate(self.lengths)]


def prompt_ids(n: int, vocab: int, seed: int) -> List[int]:
    """``n`` token ids, no tokenizer involved: every length is exact."""
    return np.random.default_rng(seed).integers(3, vocab, size=n).tolist()


FAMILIES = ("tiny-llama3.1:8b", "tiny-qwen2:1.5b", "tiny-gemma:7b", "tiny-phi3:3.8b")
STATIC = {m: Case(f"static-{m}", m, (1, 2, 33), (20, 3, 11)) for m in FAMILIES}
LLAMA = "tiny-llama3.1:8b"
CHUNKED = Case("chunked", LLAMA, (70, 9, 1, 40), (0, 0, 0, 0))
CHUNK_ROWS = (5, 16, 17, 64, None)  # CAIN_PREFILL_ROWS; None: unset
FORMATS = {(w, kv): Case(f"fmt-{w}-kv{kv}", LLAMA, (1, 20, 37), (10, 10, 10), weight_dtype=w, kv_dtype=kv)
           for w in ("fp8", "fp4", "q4_0", "q4_k", "q4_k_m") for kv in ("bf16", "fp8")}
A8 = {w: Case(f"a8-{w}", LLAMA, (1, 20, 37), (10, 10, 10), weight_dtype=w, overrides=(("d_model", 512),), a8=True,
              compare_layers=1)
      for w in ("fp8", "fp4")}
QTILE = Case("qtile-q4_k", LLAMA, (2,) * 40, (6,) * 40, weight_dtype="q4_k", max_batch=40)
FULL = Case("context-full", LLAMA, (253, 255, 4), (10, 10, 20))
# continuous batch: A, B and C admitted together, D later into A's freed slot
CONT = Case("continuous", LLAMA, (30, 5, 12, 3), (24, 3, 40, 6))
ALL_CASES: List[Case] = ([*STATIC.values(), CHUNKED, *FORMATS.values(), *A8.values(), QTILE, FULL, CONT])


# ------------------------------------------------------------------------------------------------------ the cache
def sentinel_bits(kv_dtype: str) -> torch.Tensor:
    """The sentinel as the cache stores it: one int16 (bf16) or uint8 (e4m3) element."""
    v = torch.tensor(SENTINEL[kv_dtype])
    return v.to(torch.float8_e4m3fn).view(torch.uint8) if kv_dtype == "fp8" else v.to(torch.bfloat16).view(torch.int16)


def poison(eng) -> None:
    """Both caches, all layers and all slots, filled with the sentinel."""
    for c in (eng.kcache, eng.vtcache):
        if eng.kv_dtype == "fp8":
            c.fill_(int(sentinel_bits("fp8")))
        else:
            c.fill_(SENTINEL["bf16"])
    if eng.device.type == "cuda":
        torch.cuda.synchronize(eng.device)


def read_kv(eng):
    """(K, V, kbits, vbits), each ``[layer, slot, kv head, position, head dim]``: fp32 values and the raw bits."""
    cfg = eng.cfg
    if eng.device.type == "cuda":
        eng.stream.synchronize()
        torch.cuda.synchronize(eng.device)
    L, S, H, T, hd = cfg.n_layers, eng.max_batch, cfg.n_kv_heads, eng.T_max, cfg.head_dim
    k = ops.unpack_kcache(eng.kcache.view(L, S, H, T, hd))
    v = ops.unpack_vcache(eng.vtcache.view(L, S, H, hd, T))
    if eng.kv_dtype == "fp8":
        return k.view(torch.float8_e4m3fn).float(), v.view(torch.float8_e4m3fn).float(), k, v
    return k.float(), v.float(), k.view(torch.int16), v.view(torch.int16)


def oracle_kv(ref, ids: Sequence[int], head=None, n_head: int = 0):
    """``c[layer] = [k, v]`` (``[position, kv head, head dim]`` fp32) of ``ref.forward(ids, cache=c)``: K after RoPE,
    with the e4m3 round trip when the model has ``kv_dtype="fp8"``.  With ``head``, the first ``n_head`` positions go
    through that model instead (the prefill positions of an A8 engine) and ``ref`` continues on its cache."""
    dev = ref.mw.device
    c: list = []
    if head is not None and n_head > 0:
        head.forward(torch.tensor([list(ids[:n_head])], device=dev), cache=c)
        ids = ids[n_head:]
    if len(ids):
        ref.forward(torch.tensor([list(ids)], device=dev), cache=c)
    return [[k[0].float(), v[0].float()] for k, v in c]


def expected_inputs(prompt: Sequence[int], tokens: Sequence[int], idled: bool) -> List[int]:
    """The token whose K / V each cache position of a row holds.  With prompt length L and n generated tokens,
    positions 0 .. L+n-2 are written (p_last = L+n-2): the prompt, then every generated token but the last.  A row
    that finished while its batch went on stepping keeps pos = p_last and tok = tokens[n-1] (sample.hip advance_row:
    a done row's pos stays, its tok is the last choice), and every later forward rewrites position p_last with the
    K / V of tokens[n-1] -- in place of tokens[n-2], or of the prompt's last token when n = 1.  n = 0: the prompt
    (``last_logits``)."""
    prompt, tokens = list(prompt), list(tokens)
    n = len(tokens)
    if n == 0:
        return prompt
    seq = (prompt + tokens)[: len(prompt) + n - 1]
    if idled:
        seq[-1] = tokens[-1]
    return seq


@dataclass
class Expected:
    """What the cache should hold: K, V ``[layer, slot, kv head, position, head dim]`` (fp32; only the written
    vectors mean anything) and ``written [slot, position]``."""
    K: torch.Tensor
    V: torch.Tensor
    written: torch.Tensor
    compare_layers: Optional[int] = None

    def mask(self) -> torch.Tensor:
        """[layer, slot, 1, position]: the vectors that are compared."""
        m = self.written[None, :, None, :].expand(self.K.shape[0], -1, -1, -1).clone()
        if self.compare_layers is not None:
            m[self.compare_layers:] = False
        return m


def expected_cache(ref, rows: Dict[int, Sequence[int]], slots: int, T: int = T_MAX, head=None,
                   n_head: Optional[Dict[int, int]] = None) -> Expected:
    """``rows``: {slot: the tokens at its positions 0 .. p_last}."""
    cfg, dev = ref.cfg, ref.mw.device
    shape = (cfg.n_layers, slots, cfg.n_kv_heads, T, cfg.head_dim)
    K, V = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
    written = torch.zeros(slots, T, dtype=torch.bool, device=dev)
    for s, ids in rows.items():
        c = oracle_kv(ref, ids, head, (n_head or {}).get(s, 0))
        for l, (k, v) in enumerate(c):
            K[l, s, :, : len(ids)] = k.transpose(0, 1)
            V[l, s, :, : len(ids)] = v.transpose(0, 1)
        written[s, : len(ids)] = True
    return Expected(K, V, written)


def vector_errors(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """||got - want|| / ||want|| over the head dim: ``[layer, slot, kv head, position]``."""
    return (got.float() - want.float()).norm(dim=-1) / want.float().norm(dim=-1).clamp_min(1e-30)


def layer_max(got, want: Expected) -> Tuple[List[float], List[float]]:
    """The largest error over the written vectors of each layer, for K and for V."""
    out = []
    for g, w in ((got[0], want.K), (got[1], want.V)):
        e = vector_errors(g, w) * want.mask()
        out.append([float(x) for x in e.flatten(1).amax(1)])
    return out[0], out[1]


def limits(base, want: Expected) -> Tuple[List[float], List[float]]:
    """Per layer, for K and V: MARGIN x the eager baseline's largest per-vector error, at most CAP.  ``base``: the
    baseline's (K, V) at the same positions (an ``Expected`` or a pair)."""
    b = (base.K, base.V) if isinstance(base, Expected) else base
    return tuple([min(MARGIN * x, CAP) for x in m] for m in layer_max(b, want))


def find_bad(got, want: Expected, limit):
    """[(what, layer, slot, kv head, position, error, limit)] of the written vectors over their limit, in cache order
    (K before V)."""
    bad = []
    for what, g, w, lim in (("K", got[0], want.K, limit[0]), ("V", got[1], want.V, limit[1])):
        err = vector_errors(g, w)
        lim_t = torch.tensor(lim, device=err.device, dtype=err.dtype)[:, None, None, None]
        over = (~(err <= lim_t)) & want.mask()  # a NaN error is over
        for l, s, h, p in over.nonzero().tolist():
            bad.append((what, l, s, h, p, float(err[l, s, h, p]), float(lim[l])))
    return bad


def compare(got, want: Expected, limit, tag: str = "") -> None:
    """Every written vector within its layer's limit; a failure names the count, the first and the worst vector."""
    bad = find_bad(got, want, limit)
    if bad:
        worst = max(bad, key=lambda b: b[5] if b[5] == b[5] else float("inf"))
        n = int(want.mask().sum()) * want.K.shape[2] * 2
        raise AssertionError(f"{tag}: {len(bad)} of {n} vectors over the limit; first {bad[0]}, worst {worst} "
                             f"(K or V, layer, slot, kv head, position, error, limit)")


def find_touched(bits, written: torch.Tensor, sentinel: torch.Tensor, snapshot=None, snapshot_slots=()):
    """The first (what, layer, slot, kv head, position) outside ``written`` whose bits differ from the sentinel --
    or, in ``snapshot_slots``, from the snapshot taken earlier; None when there is none."""
    for what, b, snap in (("K", bits[0], snapshot[0] if snapshot else None),
                          ("V", bits[1], snapshot[1] if snapshot else None)):
        ref = torch.full_like(b, int(sentinel))
        for s in snapshot_slots:
            ref[:, s] = snap[:, s]
        diff = (b != ref).any(-1) & ~written.to(b.device)[None, :, None, :]
        if bool(diff.any()):
            return (what, *diff.nonzero()[0].tolist())
    return None


def assert_untouched(bits, written: torch.Tensor, kv_dtype: str = "bf16", snapshot=None, snapshot_slots=(),
                     tag: str = "") -> None:
    """Every element outside (used slot, position <= that row's p_last) is bit-identical to the sentinel (to the
    snapshot in ``snapshot_slots``): all layers, and the slots no request used."""
    hit = find_touched(bits, written, sentinel_bits(kv_dtype), snapshot, snapshot_slots)
    assert hit is None, f"{tag}: cache written outside the rows' ranges, first at {hit} (K or V, layer, slot, kv head, position)"


# ------------------------------------------------------------------------------------------------------ models
def models_for(weights, case: Case):
    """(oracle, baseline, a8 baseline or None) on the weights the kernels multiply by: the fp32 oracle, the bf16
    eager baseline (tests/numerics.py) and, for an A8 case, the baseline with per-row e4m3 activations."""
    from numerics import eager_bf16

    from cain_amd.models.reference import ReferenceModel
    from cain_amd.models.weights import roundtrip_weights

    w = roundtrip_weights(weights, case.weight_dtype)
    ref = ReferenceModel(w, kv_dtype=case.kv_dtype)
    base = eager_bf16(w, kv_dtype=case.kv_dtype)
    base8 = eager_bf16(w, kv_dtype=case.kv_dtype, act_dtype="fp8") if case.a8 else None
    return ref, base, base8


def expectations(models, rows: Dict[int, Sequence[int]], slots: int, n_prefill: Optional[Dict[int, int]] = None,
                 compare_layers: Optional[int] = None):
    """(want, limits, baseline maxima) of ``rows`` ({slot: tokens at positions 0 .. p_last}); ``n_prefill``: the
    positions of each slot that an A8 engine's prefill wrote."""
    ref, base, base8 = models
    want = expected_cache(ref, rows, slots)
    want.compare_layers = compare_layers
    b = expected_cache(base, rows, slots, head=base8, n_head=n_prefill if base8 is not None else None)
    return want, limits(b, want), layer_max((b.K, b.V), want)
