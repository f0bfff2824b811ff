"""The rules of a masked search (csrc/orr_mask_plan.h) on the CPU: the in-scope sample's size, eligibility, the cost rule, the
ladder and its bound, the parts of the list path, the survivors' filter decision and the workspace slices.
build() compiles csrc/host/orr_mask_plan_selftest; this runs it.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_mask_plan_selftest")


def test_mask_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_mask_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_mask_plan_selftest: ok"


def test_the_kernels_and_the_selftest_share_their_inlines():
    """mask_survivors' per-entry decision and the part bitmap's word are written once, in the plan header; the kernels and the
    selftest call them."""
    header = open(os.path.join(CSRC, "orr_mask_plan.h")).read()
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    selftest = open(os.path.join(CSRC, "host", "orr_mask_plan_selftest.cpp")).read()
    for name, ret in (("survivor_in_scope", "bool"), ("part_word", "uint32_t")):
        assert header.count(f"inline {ret} {name}(") == 1
        assert f"mask::{name}(" in kernels and f"mask::{name}(" in selftest
        assert f" {name}(" not in kernels.replace(f"mask::{name}(", "")         # no second definition beside the kernels
    assert "mask::kMaskedRecency" in kernels


def test_the_new_entry_point_is_exported_and_documented():
    native = open(os.path.join(ROOT, "omni-recall-rag_amd", "_native.py")).read()
    assert '"orr_search_batch_masked"' in native
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md", os.path.join("include", "omnirecall_hip.h")):
        assert "orr_search_batch_masked" in open(os.path.join(ROOT, doc)).read(), doc
