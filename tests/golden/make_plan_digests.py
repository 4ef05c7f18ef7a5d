#!/usr/bin/env python3
"""Generates tests/golden/plan_digests.json, the fixture of tests/test_plan_digests.py: for every case of tests_support/plan_cases.py
(handle, dtype, toggle) the sha256 over its lines of tools/plan_fingerprint.py.  Host only.  A change that means to alter plans
regenerates the file; the diff of the JSON then names the handles that moved.

    python tests/golden/make_plan_digests.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests_support import plan_cases as PC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_digests.json"))
    args = ap.parse_args()
    lib = PC.library()
    rec = {PC.case_key(case): PC.case_digest(PC.fingerprint_lines(lib, case)) for case in PC.cases()}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases -> {args.out}")


if __name__ == "__main__":
    main()
