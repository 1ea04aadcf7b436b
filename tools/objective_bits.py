"""Regenerates tests/golden/objective_bits.json: the SHA-256 of the value and of every gradient of each evaluation of
tests/objective_bits_cases.py, with the source hash of the library that computed them.  Record it from the commit a change of the
host code must stay bit-identical to, and only again for a deliberate change of arithmetic.
usage: python tools/objective_bits.py [OUT.json]     (needs a GPU)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objective_bits_cases as oc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else oc.GOLDEN
    rec = {"library_source": oc.source_hash(), "cases": {}}
    for name, case in oc.CASES.items():
        rec["cases"][name] = oc.digests(case)
        print(name, rec["cases"][name]["value"][:16], f"({len(rec['cases'][name])} tensors)", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
