#!/usr/bin/env python3
"""Generates tests/golden/pack_digests.json, the fixture of tests/test_pack_digests.py: for every handle of
tests_support/pack_cases.py the sha256 of pack_state_dict(synthetic_state_dict(SEED)), of the manifest tuples and of the source
shapes (`host`, needs no GPU), and with --device the sha256 of the manifest regions of load_synthetic_on_device(SEED) (`device`,
on an MI355X).  The fixture records the behaviour of the commit BEFORE the front-ends were rebased onto EngineModel; it is not
to be regenerated from later code.

    python tests/golden/make_pack_digests.py [--device] [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests_support import pack_cases as PC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="add the `device` section (needs the GPU); the `host` section of an existing file is kept")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pack_digests.json"))
    args = ap.parse_args()
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rec["seed"] = PC.SEED
    if args.device:
        rec["device"] = {}
        for name, (make, _) in PC.CASES.items():
            m = make().load_synthetic_on_device(PC.SEED)
            rec["device"][name] = PC.regions_digest(m, m._weights)
    else:
        rec["host"] = {}
        for name, (make, _) in PC.CASES.items():
            m = make()
            rec["host"][name] = dict(packed=PC.sha(m.pack_state_dict(m.synthetic_state_dict(PC.SEED))), manifest=PC.manifest_digest(m),
                                     shapes=PC.shapes_digest(m), weight_bytes=int(m.weight_bytes))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
