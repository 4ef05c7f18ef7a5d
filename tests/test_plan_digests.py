"""The planner emits the plans it is recorded to emit: tests/golden/plan_digests.json holds, per case of tests_support/plan_cases.py
(handle, storage dtype, plan-rebuilding toggle), one sha256 over that handle's lines of tools/plan_fingerprint.py across the batches
(and, for T5, the sequence lengths): manifest, workspace size, FLOP sums and `ops=`, the hash over every field of every op and fold
job (sdn_debug_plan_digest).  The fixture was recorded before Builder's GEMM options moved into GemmSpec / ConvSpec, from the old
planner with only the digest hook added.  A pull request that MEANS to change plans regenerates it (tests/golden/make_plan_digests.py);
the diff of the JSON file then shows which handles moved, and tools/plan_fingerprint.py shows in which column.  Host only."""
import json
import os

import pytest

from tests_support import plan_cases as PC

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests.json")) as _f:
    GOLD = json.load(_f)
CASES = {PC.case_key(c): c for c in PC.cases()}


def test_the_fixture_covers_every_case():
    assert set(GOLD) == set(CASES)


@pytest.mark.parametrize("key", list(CASES))
def test_plans_are_the_recorded_ones(key):
    assert PC.case_digest(PC.fingerprint_lines(PC.library(), CASES[key])) == GOLD[key]
