#!/usr/bin/env python3
"""Golden fixtures of the collinear blocks.  Run HERE: needs the reference mounted at /root/reference (its
mumemto/collinear_block.py is imported from there, never copied); the fixtures are data only.

collinear/
  <table>.mums                    a seeded table (tests/collmodel.py make_table; no two kept rows share a start in a column)
  <table>.<run>.mums              written by the REAL reference tool, collinear_block.main(), from <table>.mums
  <table>.bumbl <table>.<run>.bumbl   the same through the .bumbl reader and writer, for two of the tables
  runs: g1000 = `-g 1000`, g0 = `-g 0`, g200s150 = `-g 200 --min-singleton-length 150`
"""
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), "/root/reference/mumemto"]
import collmodel  # noqa: E402
from mumemto_amd import mumsio  # noqa: E402
import collinear_block as ref_tool  # noqa: E402  (the reference's module; never copied)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "collinear")

RUNS = {"g1000": ["-g", "1000"], "g0": ["-g", "0"], "g200s150": ["-g", "200", "--min-singleton-length", "150"]}
TABLES = {
    "synteny": dict(seed=1, n=40, n_docs=3),
    "inversion": dict(seed=2, n=60, n_docs=8, inversions=[(3, 18, 29)], gaps=(0, 120, 400, 1300)),
    "moved": dict(seed=3, n=50, n_docs=4, moves=[(2, 8, 15), (3, 36, 44)]),
    "minus_column": dict(seed=4, n=40, n_docs=4, minus_cols=[2], inversions=[(1, 5, 14)]),
    "partial": dict(seed=5, n=56, n_docs=5, partial=7, inversions=[(4, 20, 36)]),
    "unsorted": dict(seed=6, n=48, n_docs=4, shuffle=True, moves=[(1, 3, 11)], inversions=[(3, 25, 34)], partial=3),
}
BUMBL = ("inversion", "unsorted")


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for name, spec in TABLES.items():
        lengths, starts, strands = collmodel.make_table(**spec)
        collmodel.assert_no_ties(starts)
        inputs = [os.path.join(OUT, name + ".mums")]
        open(inputs[0], "wb").write(collmodel.mums_bytes(lengths, starts, strands))
        if name in BUMBL:
            inputs.append(os.path.join(OUT, name + ".bumbl"))
            mumsio.write_bumbl(inputs[1], lengths, starts, strands)
        for src in inputs:
            ext = os.path.splitext(src)[1]
            for run, flags in RUNS.items():
                dst = os.path.join(OUT, "%s.%s%s" % (name, run, ext))
                ref_tool.main(ref_tool.parse_arguments(["-m", src, "-o", dst] + flags))
                assert os.path.exists(dst), dst
        got = mumsio.read_mums(os.path.join(OUT, name + ".g1000.mums"), with_blocks=True)
        print("%-13s %3d rows in, %3d kept, %d blocks at -g 1000" % (name, len(lengths), len(got[0]),
                                                                      len(set(got[3].tolist()) - {mumsio.NO_BLOCK})))


if __name__ == "__main__":
    main()
