"""The step entries refuse a bad call record before any HIP call (CPU-only: host pointers, the null stream).

A refusal is -1 from ``cain_step_run``, and a null graph with ``err == -1`` from ``cain_step_capture``; a launch or a
capture attempted without a GPU would return a HIP error code instead, so the values are asserted, not merely that
they are non-zero.  Only refusals are asserted: a well-formed record is never handed to an entry, which would launch
on the host pointers where a GPU is present.  Each case is a complete record with one defect.
"""
import ctypes

import pytest

from cain_amd import ops

_buf = (ctypes.c_char * 64)()  # stands for every buffer: no entry may read or launch on it
P = ctypes.addressof(_buf)
PLAN_ROWS = 8


@pytest.fixture(scope="module")
def plan():
    """A plan of no layers for forwards of up to 8 rows over a vocabulary of one token (no chunk-maxima buffer)."""
    lib = ops.load()
    desc = ops.CainPlanDesc(n_layers=0, Mpad=PLAN_ROWS, V=1)
    handle = lib.cain_plan_create(ctypes.byref(desc))
    assert handle
    yield handle
    lib.cain_plan_destroy(ctypes.c_void_p(handle))


def _filled(cls, **ints):
    """A record whose every pointer is the host buffer and whose integers are 0, but for ``ints``."""
    rec = cls()
    for name, typ in cls._fields_:
        setattr(rec, name, P if typ is ctypes.c_void_p else 0)
    for k, v in ints.items():
        setattr(rec, k, v)
    return rec


def _complete(plan, *feats):
    """A well-formed step over 2 rows of ``plan`` with the records ``feats`` names (``step.parts`` holds them): with
    ``spec`` a speculative step over 2 sequences of one draft each, with ``spec_draft`` one a draft model proposes
    (the draft plans: the plan itself)."""
    parts = dict(rows=_filled(ops.CainRows, ldg=1))
    if "lp" in feats:
        parts["lp"] = _filled(ops.CainLogprob)
    if "gr" in feats:
        parts["gr"] = _filled(ops.CainGrammar)
    if "st" in feats:
        parts["st"] = _filled(ops.CainStop)
    if "spec" in feats:
        parts["spec"] = _filled(ops.CainSpec, K=1, mode=int("spec_draft" in feats), slots=1, lds=1, ldv=1, ldt=1,
                                vocab=1, ldg=1)
    if "spec_draft" in feats:
        parts["spec_draft"] = _filled(ops.CainSpecDraft, K=1, dvocab=1, dbos=0, slots=1, lds=1, ldv=1, ldg=1)
    step = ops.CainStep(plan=plan, M=2, want_logits=1, want_sample=1)
    if "spec_draft" in feats:
        step.draft2 = step.draft1 = plan
    for name, rec in parts.items():
        setattr(step, name, ctypes.pointer(rec))
    step.parts = parts
    return step


def _field(name, value):
    return lambda step: setattr(step, name, value)


def _part(part, name, value):
    return lambda step: setattr(step.parts[part], name, value)


# name: (the records of the complete step, its one defect)
CASES = {
    "null rows": ((), _field("rows", None)),
    "M = 0": ((), _field("M", 0)),
    "M above the plan's rows": ((), _field("M", PLAN_ROWS + 1)),
    "lp without logits": (("lp",), _field("want_logits", 0)),
    "lp with a null topn": (("lp",), _part("lp", "topn", None)),
    "gr without the sampler": (("gr",), _field("want_sample", 0)),
    "gr with a null gstate": (("gr",), _part("gr", "gstate", None)),
    "st with a null stop_bytes": (("st",), _part("st", "stop_bytes", None)),
    "st with a null rows.gen": (("st",), _part("rows", "gen", None)),
    "spec with K = 0": (("spec",), _part("spec", "K", 0)),
    "spec with K above the limit": (("spec",), _part("spec", "K", ops.SPEC_K_MAX + 1)),
    "spec with lp": (("spec", "lp"), None),
    "spec with gr": (("spec", "gr"), None),
    "spec with st": (("spec", "st"), None),
    "spec_draft without spec": (("spec", "spec_draft"), _field("spec", None)),
    "spec_draft with an n-gram spec": (("spec", "spec_draft"), _part("spec", "mode", 0)),
    "spec_draft with a null draft2": (("spec", "spec_draft"), _field("draft2", None)),
}


def _capture(step, steps):
    err = ctypes.c_int(0)
    graph = ops.load().cain_step_capture(ctypes.byref(step) if step is not None else None, steps, None,
                                         ctypes.byref(err))
    return graph, err.value


@pytest.mark.parametrize("case", list(CASES))
def test_both_entries_refuse(plan, case):
    feats, defect = CASES[case]
    step = _complete(plan, *feats)
    if defect is not None:  # (else the combination of records is the defect)
        defect(step)
    assert ops.load().cain_step_run(ctypes.byref(step), None) == -1
    assert _capture(step, 1) == (None, -1)


def test_capture_refuses_no_steps(plan):
    assert _capture(_complete(plan), 0) == (None, -1)


def test_null_record_and_null_plan_refused(plan):
    assert ops.load().cain_step_run(None, None) == -1
    assert _capture(None, 1) == (None, -1)
    step = _complete(plan)
    step.plan = None
    assert ops.load().cain_step_run(ctypes.byref(step), None) == -1
    assert _capture(step, 1) == (None, -1)
