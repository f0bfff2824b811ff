"""The rules of a grouped masked search (csrc/orr_group_plan.h) on the CPU: a group's sample size with its buffer term and its
cap, the split into screen and list groups, the summed cost rule, the one-used-group shortcut, the ladder's next step and its
bound, the workspace slice.  build() compiles csrc/host/orr_group_plan_selftest; this runs it.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-recall-rag_amd")
CSRC = os.path.join(PKG, "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_group_plan_selftest")


def test_group_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_group_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_group_plan_selftest: ok"


def test_the_grouped_filter_shares_the_masked_filters_decision():
    """mask_survivors_grouped decides per entry as mask_survivors does: through mask::survivor_in_scope, which stays the one
    definition; the row constants use it too, and both new kernels are launched under a timed name of their own."""
    kernels = open(os.path.join(CSRC, "orr_kernels.hip")).read()
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    for kernel in ("mask_survivors_grouped_kernel", "row_consts_grouped_kernel"):
        body = kernels[kernels.index("void " + kernel + "("):]
        body = body[:body.index("\nhipError_t ")]
        assert "mask::survivor_in_scope(" in body, kernel
    assert open(os.path.join(CSRC, "orr_mask_plan.h")).read().count("inline bool survivor_in_scope(") == 1
    assert "survivor_in_scope" not in open(os.path.join(CSRC, "orr_group_plan.h")).read().replace("mask::survivor_in_scope", "")
    for name in ("row_consts_grouped", "mask_survivors_grouped"):
        assert re.search(r'Timed t\(idx, [^;]*"%s"' % name, api), name
    # the plan the driver runs is the header's
    for fn in ("group::plan(", "group::next_step(", "group::screen_slice(", "group::pass_cap(", "group::groups_valid(", "group::assignment_valid("):
        assert fn in api, fn


def test_the_new_entry_point_is_exported_and_documented():
    native = open(os.path.join(PKG, "_native.py")).read()
    assert '"orr_search_batch_masked_groups"' in native and "hip.orr_search_batch_masked_groups.argtypes" in native
    assert "def search_masked_groups(" in open(os.path.join(PKG, "index.py")).read()
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md", os.path.join("include", "omnirecall_hip.h")):
        assert "orr_search_batch_masked_groups" in open(os.path.join(ROOT, doc)).read(), doc
    header = open(os.path.join(ROOT, "include", "omnirecall_hip.h")).read()
    assert "#define ORR_ABI_VERSION 1" in header.replace("  ", " ")              # adding a function is compatible
    assert "6 two-stage screen" in " ".join(header.split())                       # pass_mode 6 in orr_search_stats' comment
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_group_plan_selftest" in makefile.split("all:")[0]            # in the SELFTEST list: build() makes it
