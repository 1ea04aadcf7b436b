"""Regenerates one section of tests/golden/score_refusals.json: what every bad call of tests/score_refusal_cases.py raises, as
"{type name}: {message}".  Record it from the commit a change of the host code must keep every refusal of, word for word and in the
same order.  The other section of the file is kept as it is.
usage: python tools/score_refusals.py host [OUT.json]            (CPU models: needs no GPU)
       python tools/score_refusals.py post_cross [OUT.json]      (device operands: needs a GPU; nothing is launched)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_refusal_cases as rc  # noqa: E402


def main():
    section = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else rc.GOLDEN
    cases = {"host": rc.HOST_CASES, "post_cross": rc.POST_CROSS_CASES}[section]
    rec = {}
    if os.path.exists(rc.GOLDEN):
        with open(rc.GOLDEN) as f:
            rec = json.load(f)
    rec[section] = {name: rc.record(case) for name, case in cases.items()}
    for name, what in rec[section].items():
        print(f"{name:70s} {what}", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
