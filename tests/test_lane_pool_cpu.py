"""The lane pool's protocol (omni-recall-rag_amd/csrc/orr_lanes.h) on the CPU: host/orr_lanes_selftest runs one scenario per call
against an empty orr_index of its own -- no HIP, no GPU.  Every wait in the binary has a deadline (a watchdog ends it with exit
status 3), and the subprocess time limit here stands behind that, so a broken protocol fails; it does not hang."""
import os
import subprocess

import pytest

from helpers import ROOT

SELFTEST = os.path.join(ROOT, "omni-recall-rag_amd", "csrc", "host", "orr_lanes_selftest")

SCENARIOS = [
    "more_threads_than_lanes",        # 16 threads on 4 lanes: at most 4 held, one holder per lane, at most 3 views made
    "exclusive_against_creation",     # Exclusive waits for a lane being made; no lane is made while it is held
    "exclusive_against_searches",     # nothing is held inside Exclusive; a lane made just before it has one holder at a time
    "make_fails",                     # max_lanes falls to the lanes there are; the failed slot is never handed out
    "drain_and_regrowth",             # drain() returns exactly the views made; the pool grows again afterwards
    "ordered_acquisition",            # 6 threads x 3 one-lane pools through acquire_in_order: all finish
]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_lane_pool_scenario(scenario):
    assert os.path.exists(SELFTEST), "build() makes %s" % SELFTEST
    done = subprocess.run([SELFTEST, scenario], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (scenario, done.returncode, done.stdout, done.stderr)
    assert done.stdout.strip() == scenario + " ok"


def test_the_binary_knows_exactly_these_scenarios():
    done = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2
    assert [line.strip() for line in done.stderr.splitlines()[1:]] == SCENARIOS
