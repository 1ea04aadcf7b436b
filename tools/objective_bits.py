"""Regenerates the golden file of a module of bit-for-bit cases: the SHA-256 of every tensor each of its evaluations returns, with the
source hash of the library that computed them.  The modules: tests/objective_bits_cases.py (the default; the value and every gradient
of each training objective, tests/golden/objective_bits.json) and tests/score_bits_cases.py (the candidate scores,
tests/golden/score_bits.json).  Record it from the commit a change of the host code must stay bit-identical to, and only again for a
deliberate change of arithmetic.
usage: python tools/objective_bits.py [MODULE] [OUT.json]     (needs a GPU; MODULE: objective_bits_cases or score_bits_cases)"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    args = sys.argv[1:]
    module = args.pop(0) if args and not args[0].endswith(".json") else "objective_bits_cases"
    oc = importlib.import_module(module)
    out = args[0] if args else oc.GOLDEN
    rec = {"library_source": oc.source_hash(), "cases": {}}
    for name, case in oc.CASES.items():
        rec["cases"][name] = oc.digests(case)
        print(name, next(iter(rec["cases"][name].values()))[:16], f"({len(rec['cases'][name])} tensors)", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
