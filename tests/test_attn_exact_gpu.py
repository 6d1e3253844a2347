"""Decode attention (csrc/attention.hip) against the exact cases of ``tests/attn_exact.py``: one-hot, uniform and
power-of-two-weight rows whose output is known bit for bit (module doc there), on every register body, both merge
widths, every split-merge body and the LDS-ring kernel.

One launch covers a handful of rows, each with its own length and slot (a permutation into rows + 3 slots, every
unused position and slot poisoned), one idle row, ``out`` a view of a wider buffer whose pad columns must keep
their sentinel, ``part_o`` / ``part_ml`` at exactly the documented sizes between canaries, and the whole nsplit list
run twice on one ``counters`` tensor that must end all zero.  A failure names (row, query head, kv head, 16-dim
tile) and, for the one-hot family, the position whose V row came out.

The parametrize ids say which path of ``cain_attention_ex`` and which merge of ``attn_decode_kernel`` a geometry
forces (``attn_exact.Geo``); head_dim 256 always runs its own one-set body, whatever body is selected."""
import functools
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, str(Path(__file__).parent))

import attn_exact as ax  # noqa: E402
from cain_amd import ops  # noqa: E402

DEV = torch.device("cuda")
GUARD = 1024  # canary floats on each side of part_o and part_ml
CANARY = -7.25
BODIES = {2: "body2-oneset-4persimd", 1: "body1-oneset-3persimd", 0: "body0-pingpong"}


@functools.lru_cache(maxsize=None)
def _case(l: ax.Launch, fam: str, kv8: bool):
    """The device tensors of one (launch, family, cache type), made once and never written."""
    d = ax.make(l, fam, kv8)
    q, kp, vp = ax.pack(d)
    slot = torch.tensor(l.slot, device=DEV, dtype=torch.int32)
    pos = torch.tensor([max(L - 1, 0) for L in l.lengths], device=DEV, dtype=torch.int32)
    return dict(q=q.to(DEV), kp=kp.to(DEV), vp=vp.to(DEV), slot=slot, pos=pos, want=d.want.bfloat16().to(DEV),
                alt=d.alt.bfloat16().to(DEV), scale=d.scale, kscale=d.kscale, vscale=d.vscale)


class _Run:
    """Launches now, verdicts later: every check stays on the device until ``finish`` (one synchronisation)."""

    def __init__(self):
        self.items = []

    def launch(self, l: ax.Launch, fam: str, kv8: bool, nsplit: int, counters: torch.Tensor, tag: str):
        g, c = l.geo, _case(l, fam, kv8)
        n = g.H * g.hd
        full = torch.full((g.rows, n + 64), ax.SENTINEL, device=DEV, dtype=torch.bfloat16)
        n_o = g.rows * g.H * nsplit * g.hd
        n_ml = ops.attention_ml_floats(g.rows, g.H, g.Hkv, nsplit)
        ws = torch.full((3 * GUARD + n_o + n_ml,), CANARY, device=DEV, dtype=torch.float32)
        part_o, part_ml = ws[GUARD:GUARD + n_o], ws[2 * GUARD + n_o:2 * GUARD + n_o + n_ml]
        ops.attention(c["q"], c["kp"], c["vp"], c["slot"], c["pos"], g.H, g.Hkv, g.hd, nsplit, c["scale"],
                      out=full[:, :n], part_o=part_o, part_ml=part_ml, counters=counters, kscale=c["kscale"],
                      vscale=c["vscale"])
        o = full[:, :n].reshape(g.rows, g.H, g.hd)
        guards = torch.cat([ws[:GUARD], ws[GUARD + n_o:2 * GUARD + n_o], ws[2 * GUARD + n_o + n_ml:]])
        ok = torch.stack([((o == c["want"]) | (o == c["alt"])).all(), (full[:, n:] == ax.SENTINEL).all(),
                          (guards == CANARY).all()])
        self.items.append((ok, full, (l, fam, kv8), f"{tag} nsplit {nsplit}"))

    def counters_zero(self, counters: torch.Tensor, tag: str):
        z = (counters == 0).all()
        self.items.append((torch.stack([z, z, z]), None, None, f"{tag}: counters not reset"))

    def finish(self):
        oks = torch.stack([it[0] for it in self.items]).cpu()
        for (okd, full, key, tag), ok in zip(self.items, oks):
            if bool(ok.all()):
                continue
            assert full is not None, tag
            l, fam, kv8 = key
            n = l.geo.H * l.geo.hd
            assert bool(ok[1]), f"{tag}: the pad columns of out (ldo = H hd + 64) were written"
            assert bool(ok[2]), f"{tag}: part_o / part_ml written outside their documented sizes"
            ax.assert_equal(ax.make(l, fam, kv8), full[:, :n], tag)
        self.items = []


@pytest.mark.parametrize("body", list(BODIES), ids=list(BODIES.values()))
@pytest.mark.parametrize("g", ax.GEOS, ids=lambda g: g.id)
def test_attention_exact(g, body):
    """(a) and (b) bit for bit, (c) to the admissible bf16 neighbour(s), on bf16 and fp8 caches."""
    run = _Run()
    try:
        ops.set_attention_body(body)
        for l in ax.launches(g):
            for kv8 in (False, True):
                for fam in ax.FAMILIES:
                    counters = torch.zeros(g.rows * g.Hkv, device=DEV, dtype=torch.int32)
                    tag = f"{BODIES[body]} {fam} {'fp8' if kv8 else 'bf16'}"
                    for nsplit in g.nsplits * 2:  # twice on the same counters: the reducer resets them
                        run.launch(l, fam, kv8, nsplit, counters, tag)
                    run.counters_zero(counters, f"{l.id} {tag}")
    finally:
        ops.set_attention_body(2)  # the default
    run.finish()


@pytest.mark.parametrize("g", ax.RING_GEOS, ids=lambda g: g.id)
def test_attention_ring_exact(g):
    """The LDS-ring body on a persistent grid of 8 workgroups, against the exact expectation: 16 pairs (2 per CU,
    the lower edge), 512 pairs (every compute wave walks all 16 schedule entries; idle rows on the first, a middle
    and the last entry of one wave's list), and 15 / 513 pairs, which cain_attention_ex hands to the register
    kernel.  Idle rows come out as zeros on either path, so the fall-back shows only in its being exact too."""
    run = _Run()
    try:
        ops.set_cu_budget(ax.RING_CU)
        ops.set_attention_ring(1)
        for l in ax.launches(g):
            for fam in ax.FAMILIES:
                counters = torch.zeros(g.rows * g.Hkv, device=DEV, dtype=torch.int32)
                for _ in range(2):
                    run.launch(l, fam, False, 1, counters, f"ring budget {ax.RING_CU} {fam}")
    finally:
        ops.set_cu_budget(0)
        ops.set_attention_ring(1)  # the default
    run.finish()
