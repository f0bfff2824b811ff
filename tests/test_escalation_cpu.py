"""The escalation ladder (omni-recall-rag_amd/csrc/orr_escalation.h) on the CPU: which pass the uncertified queries of a batch go
through next, for one index and for the shards of a cluster.  host/orr_escalation_selftest runs one scenario per call on plain
data -- no HIP, no GPU, no index."""
import os
import subprocess

import pytest

from helpers import ROOT

SELFTEST = os.path.join(ROOT, "omni-recall-rag_amd", "csrc", "host", "orr_escalation_selftest")

SCENARIOS = [
    "rungs_in_order",                 # one shard: GrowBuffers with grown_survivor_cap's cap, Unfused, Exact, WiderK = min(n, 4 k'), Exhausted, Done
    "mixed_causes",                   # an uncertified query that did not overflow: no GrowBuffers
    "growth_refused",                 # 2^19 survivors, half of the rows, buffers of 2 GiB: the next rung instead
    "three_shards",                   # overflow on one shard; growth possible on one and refused on another; a shard without a two-stage pass
    "repeat_only_if_grown",           # pass_cap < survivor_cap and cap <= survivor_cap: one index repeats the pass, a cluster does not
    "termination",                    # fed "still uncertified", every ladder ends within kMaxRepeats; the longest takes exactly that
    "old_against_new",                # the decision parts of the two functions decide() replaced, over an exhaustive small grid
    "survivors_accounted",            # account_survivors against hand-computed totals
    "slices_and_first_kprime",        # slice_width at the boundary of kPassWorkspaceBytes; initial_kprime
    "stats_added",                    # add_search_stats: every field of orr_search_stats summed, maximised or left alone on purpose
]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_escalation_scenario(scenario):
    assert os.path.exists(SELFTEST), "build() makes %s" % SELFTEST
    done = subprocess.run([SELFTEST, scenario], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (scenario, done.returncode, done.stdout, done.stderr)
    assert done.stdout.strip() == scenario + " ok"


def test_the_binary_knows_exactly_these_scenarios():
    done = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2
    assert [line.strip() for line in done.stderr.splitlines()[1:]] == SCENARIOS
