"""Fingerprint of everything the host-side planner decides, for checking that a change to csrc/sdn_plan*.hip leaves the plans alone.

For the handles of tests_support/plan_cases.py (the configurations the host tests create, at every storage dtype their creators
accept, the UNet ones under every plan-rebuilding toggle) it prints one line per (handle, toggle, batch), and for T5 per sequence
length: parameter count, SHA-256 over every sdn_param_info, weight bytes, workspace bytes, FLOPs and their attention share, and
`ops=`: sdn_debug_plan_digest's 64-bit FNV-1a over the plan header, every field of every op and the handle's fold jobs.  The first
columns show WHAT moved (manifest, arena peak, FLOP sums); the last one shows that something did, down to a flag that went from one
GEMM to its neighbour.  Host only: no GPU is touched.  Compare two builds by running each in a process of its own and diffing:

    SDN_LIB=/path/to/old/libsdn.so python tools/plan_fingerprint.py > old.txt
    python tools/plan_fingerprint.py > new.txt && diff old.txt new.txt

tests/test_plan_digests.py pins one SHA-256 per handle over these lines (tests/golden/plan_digests.json).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests_support import plan_cases as PC  # noqa: E402


def main():
    lib = PC.library()
    for case in PC.cases():
        print("\n".join(PC.fingerprint_lines(lib, case)))


if __name__ == "__main__":
    main()
