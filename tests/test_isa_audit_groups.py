"""tests/test_isa_audit.py's proof for attn_w64_groups.hip: the grouped instantiations of attn_w64_kernel's body name the accumulator
registers a[0:255] literally as well, so there too the compiler must never touch the accumulator file or M0, spill nothing and use no
scratch -- and the translation unit holds exactly the two grouped kernels (attn_w64.hip keeps exactly its two)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "mmpl_amd", "csrc")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_attn_w64_groups_owns_the_accumulator_file(tmp_path):
    import audit_w64
    problems, info = audit_w64.audit(str(tmp_path), os.path.join(CSRC, "attn_w64_groups.hip"))
    assert not problems, problems
    assert info["agpr_count"] == [256, 256] and all(v <= 512 for v in info["vgpr_count"])
