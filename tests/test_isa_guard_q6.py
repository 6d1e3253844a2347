"""gemm_qstream.hip's Q6_K stream kernels keep their counted load waits in the BUILT library (CPU-only check), as
tests/test_isa_guard.py holds its Q4 instances to: every q6_stream_kernel instance has a loop, and at most Q4_LIMIT[epi]
``s_waitcnt vmcnt(0)`` in its loops -- the project's bound for the same loop shape (the ring, the activation
staging's gain loads, the epilogue's loads at a tile edge).  Only wait counts are read."""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

import isa_guard  # noqa: E402

# tests/test_isa_guard.py Q4_LIMIT: EPI -> the most vmcnt(0) a GGUF stream kernel's loops may hold
Q4_LIMIT = {0: 9, 1: 9, 2: 5, 3: 5, 4: 5, 5: 21}


def test_q6_stream_kernels_keep_counted_waits():
    if not (isa_guard.LLVM / "llvm-objdump").exists() or shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists():
        pytest.skip("ROCm llvm tools not available")
    from cain_amd import build

    lib = build.build_kernels()
    found = {}
    for co in isa_guard.code_objects(lib):
        found.update(isa_guard.kernel_loop_waits(isa_guard.disassemble(co), "q6_stream_kernel"))
    # 3 epilogues x 2 wave counts x 2 norms, + the 4-wave QKV pair
    assert len(found) == 14, sorted(found)
    for name, (n_loop, waits) in found.items():
        m = re.search(r"q6_stream_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E", name)
        assert m, name
        waves, u, epi, norm = (int(x) for x in m.groups())
        assert n_loop > 0, f"{name}: no loop found"
        assert waits <= Q4_LIMIT[epi], f"{name}: {waits} vmcnt(0) in its loops (limit {Q4_LIMIT[epi]})"
        assert not (epi == 5 and waves == 8), name
