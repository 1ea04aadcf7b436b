"""Regenerates tests/golden/dag_tile_pipeline_sha.json: the SHA-256 of the factor the ticket list leaves at each size of
tests/dag_tile_cases.py, from whatever build of the library the tree holds (record it from the commit a change must stay
bit-identical to; profiles/EXPERIMENTS.md names the commit the stored file came from).
usage: python tools/dag_tile_sha.py [OUT.json]     (needs a GPU)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dag_tile_cases as dc  # noqa: E402
from gpplus_amd.backend import OPT_COOP_PANEL, get_context  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else dc.GOLDEN
    ctx = get_context("cuda:0")
    ctx.set_option(OPT_COOP_PANEL, 1)
    sha = {}
    for n in dc.SIZES:
        A, _ = dc.factor_and_inverse(ctx, n, list_on=True)
        rows, inv_rows, ntasks, abort, tickets = dc.list_state(ctx)
        assert rows == n and inv_rows == n and abort == 0 and tickets >= ntasks > 0, (rows, inv_rows, ntasks, abort, tickets)
        sha[str(n)] = dc.factor_sha256(A, n)
        print(n, sha[str(n)], f"({ntasks} tasks, {tickets} tickets)", flush=True)
        del A
    print("library:", ctx.lib.gpp_version().decode())
    with open(out, "w") as f:
        json.dump(sha, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
