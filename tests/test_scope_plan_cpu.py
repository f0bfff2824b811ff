"""The rules of a scoped search (csrc/orr_scope_plan.h) on the CPU: form choice, the ladder's end, slices that cover every query
exactly once, offset validation, and the bitmap clip -- the inline the compaction kernel shares -- against a scalar restatement.
build() compiles csrc/host/orr_scope_plan_selftest; this runs it.  No GPU."""
import os
import subprocess

from helpers import ROOT

SELFTEST = os.path.join(ROOT, "omni-recall-rag_amd", "csrc", "host", "orr_scope_plan_selftest")


def test_scope_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_scope_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "orr_scope_plan_selftest: ok"
    assert "FAILED" not in r.stdout


def test_the_kernel_and_the_selftest_share_one_clip():
    """The compaction kernel calls the header's clip_word; it has no copy of its own."""
    csrc = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
    kernels = open(os.path.join(csrc, "orr_kernels.hip")).read()
    header = open(os.path.join(csrc, "orr_scope_plan.h")).read()
    assert "scope::clip_word(" in kernels
    assert header.count("inline uint32_t clip_word(") == 1 and "clip_word" in open(os.path.join(csrc, "host", "orr_scope_plan_selftest.cpp")).read()
