"""The rules of a scoped / masked search over a cluster's shards (csrc/orr_cluster_scope_plan.h) on the CPU: the split of the
global candidate_limit into per-shard counts, the ladder and its bound, the slices of a merge.
build() compiles csrc/host/orr_cluster_scope_plan_selftest; this runs it.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omni-recall-rag_amd", "csrc")
SELFTEST = os.path.join(CSRC, "host", "orr_cluster_scope_plan_selftest")


def test_cluster_scope_plan_selftest_passes():
    assert os.path.exists(SELFTEST), "build() makes it (csrc/Makefile, target host/orr_cluster_scope_plan_selftest)"
    r = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "orr_cluster_scope_plan_selftest: ok"


def test_the_library_calls_the_rules_and_does_not_restate_them():
    api = open(os.path.join(CSRC, "orr_api.hip")).read()
    assert '#include "orr_cluster_scope_plan.h"' in api
    for name in ("split_limit", "shard_limit", "first_rung", "next_rung", "merge_slice", "kMaxRungs"):
        assert f"cscope::{name}" in api, name
    header = open(os.path.join(CSRC, "orr_cluster_scope_plan.h")).read()
    assert "__global__" not in header and "hip" not in header.lower().replace("orr_search_shard_masked", "")      # host-only
    # the split is written once: no second max(0, max(1, limit) - before) beside the header's in the cluster's code
    cluster_part = api[api.index("struct ClusterScope"):]
    assert not re.search(r"candidate_limit\)\s*-", cluster_part)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "host/orr_cluster_scope_plan_selftest" in makefile.split("all:")[0]                                     # in SELFTEST
