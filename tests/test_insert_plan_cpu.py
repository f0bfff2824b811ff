"""The merge plan of orr_index_insert_rows (omni-recall-rag_amd/csrc/orr_insert_plan.h) on the CPU: where the new rows of a
sealed shard go, how far the old rows move, where the deleted rows end up, and the merged token index.
host/orr_insert_plan_selftest runs one scenario per call on plain data -- no HIP, no GPU, no index -- and checks the merged
order against std::stable_sort over old-then-new and the merged token map against build_token_index over the merged contents."""
import os
import subprocess

import pytest

from helpers import ROOT

SELFTEST = os.path.join(ROOT, "omni-recall-rag_amd", "csrc", "host", "orr_insert_plan_selftest")

SCENARIOS = [
    "front",                          # every new row newer than the shard: every old row moves
    "middle",                         # insertion points inside the shard, two new rows at one tick
    "back",                           # every new row older: nothing moves; negative ticks
    "ties",                           # new rows at the ticks of old rows go behind them and keep their own order
    "empty_old",                      # a sealed shard without rows
    "empty_new",                      # nothing to insert
    "all_equal",                      # one tick everywhere
    "no_content",                     # rows without content; an old shard without a single token
    "token_lengths",                  # tokens of 1, 16, 17, 32, 33 and 200 bytes, old and new
    "unicode_whitespace",             # the whitespace set of char.IsWhiteSpace in UTF-8; U+200B is none
    "deleted_rows",                   # the deleted positions follow their rows
    "loaded_tombstones",              # a loaded shard's mirror has 0 at deleted positions: repaired before the plan reads it
    "many_rows",                      # 9,000 + 700 pseudo-random rows: the token index is built by several threads
]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_insert_plan_scenario(scenario):
    assert os.path.exists(SELFTEST), "build() makes %s" % SELFTEST
    done = subprocess.run([SELFTEST, scenario], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (scenario, done.returncode, done.stdout, done.stderr)
    assert done.stdout.strip() == scenario + " ok"


def test_the_binary_knows_exactly_these_scenarios():
    done = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=120)
    assert done.returncode == 2
    assert [line.strip() for line in done.stderr.splitlines()[1:]] == SCENARIOS
