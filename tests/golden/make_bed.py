#!/usr/bin/env python3
"""Golden fixtures of the BED writer.  Run HERE: needs the reference mounted at /root/reference (its mumemto/mum_to_bed.py and
mumemto/collinear_block.py are imported from there, never copied); the fixtures are data only.

The reference package's __init__ imports a compiled core, so an empty module `mumemto` whose __path__ is the reference's
package directory is registered before the import: its pure-Python modules load, its __init__ never runs.

bed/
  <table>.mums                      a seeded table (tests/collmodel.py make_table)
  <table>.<run>.mums                written by the reference's collinear_block tool from it: g1000 = `-g 1000`, g0 = `-g 0`
  <table>.lengths                   a made-up multi-FASTA lengths file (the reference does not open the paths in it)
  <table>.<run>.s<K>.L<N>.bed       written by the reference's mum_to_bed tool: -s K -L N; K = 0, 1, the last column, and
                                    the column of inversion's inverted segment and minus_column's '-' column
  partial.mums, partial.s<K>.L<N>.bed   a table without blocks and with partial rows, recorded with -v

Contigs: synteny one per sequence; inversion three; moved forty; minus_column contigs of length 0 at the start and in the
middle, and in every sequence a boundary exactly on the begin of a record; partial five.  No table holds a one-row block
(the reference crashes on them); inversion.g1000 and moved.g1000 end in a free row, the other tables in a block.
"""
import contextlib
import io
import os
import shutil
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = types.ModuleType("mumemto")
pkg.__path__ = ["/root/reference/mumemto"]
sys.modules["mumemto"] = pkg
import numpy as np  # noqa: E402
import bedmodel  # noqa: E402
import collmodel  # noqa: E402
from mumemto_amd import mumsio  # noqa: E402
from mumemto_amd.find_inversions import blocks_of_rows  # noqa: E402
from mumemto import collinear_block as ref_collinear  # noqa: E402  (the reference's modules; never copied)
from mumemto import mum_to_bed as ref_bed  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bed")
RUNS = {"g1000": ["-g", "1000"], "g0": ["-g", "0"]}
TABLES = {
    "synteny": dict(seed=1, n=40, n_docs=3),
    "inversion": dict(seed=2, n=60, n_docs=8, inversions=[(3, 18, 29)], gaps=(0, 120, 400, 1300)),
    "moved": dict(seed=3, n=50, n_docs=4, moves=[(2, 8, 15), (3, 36, 44)]),
    "minus_column": dict(seed=4, n=40, n_docs=4, minus_cols=[2], inversions=[(1, 5, 14)]),
}
PARTIAL = dict(seed=5, n=56, n_docs=5, partial=7, inversions=[(4, 20, 36)])
MIN_SINGLE = (100, 0)
EXTRA_COLUMNS = {"inversion": [3], "minus_column": [2]}       # beside 0, 1 and the last: the inverted segment, the '-' column


def split(total, count, rng):
    cuts = np.sort(rng.choice(np.arange(1, total), count - 1, replace=False)) if count > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate(([0], cuts, [total]))).tolist()


def contig_lengths(name, table, blocks, rng):
    lengths, starts, _ = table
    out = []
    for c in range(starts.shape[1]):
        total = int((starts[:, c] + lengths.astype(np.int64)).max()) + 1 + int(rng.integers(0, 500))
        if name == "synteny":
            lens = [total]
        elif name == "inversion":
            lens = split(total, 3, rng)
        elif name == "moved":
            lens = split(total, 40, rng)
        elif name == "partial":
            lens = split(total, 5, rng)
        else:                      # minus_column: zeros at the start and in the middle, a boundary on the begin of a record
            begin = bedmodel.intervals(*table, c, 0, blocks)[0]
            at = int(np.sort(begin)[len(begin) // 2])
            lens = [0, 0] + split(at, 2, rng) + [0] + split(total - at, 3, rng)
            assert at in np.cumsum(lens).tolist()
        assert sum(lens) == total
        out.append(lens)
    return out


def write_lengths(path, name, lens):
    with open(path, "w") as f:
        for c, seq in enumerate(lens):
            fasta = "/data/genomes/%s_%d.fa" % (name, c)
            f.write("%s * %d\n" % (fasta, sum(seq)))
            for k, v in enumerate(seq):
                f.write("%s %s_%d_ctg%d %d\n" % (fasta, name, c, k, v))


def record(argv, dst):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ref_bed.main(ref_bed.parse_arguments(argv + ["-o", dst]))       # (on stdout the tool closes the stream it is given)
    return open(dst).read().count("\n")


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    rng = np.random.default_rng(77)
    for name, spec in TABLES.items():
        table = collmodel.make_table(**spec)
        collmodel.assert_no_ties(table[1])
        src = os.path.join(OUT, name + ".mums")
        open(src, "wb").write(collmodel.mums_bytes(*table))
        lens_path = os.path.join(OUT, name + ".lengths")
        for run, flags in RUNS.items():
            dst = os.path.join(OUT, "%s.%s.mums" % (name, run))
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                ref_collinear.main(ref_collinear.parse_arguments(["-m", src, "-o", dst] + flags))
            got = mumsio.read_mums(dst, with_blocks=True)
            blocks = blocks_of_rows(got[3])
            assert len(blocks) and (blocks[:, 1] > blocks[:, 0]).all(), "a one-row block in %s" % dst
            if run == "g1000":
                write_lengths(lens_path, name, contig_lengths(name, got[:3], blocks, rng))
            last = got[0].shape[0] - 1
            for s in sorted({0, 1, got[1].shape[1] - 1} | set(EXTRA_COLUMNS.get(name, []))):
                for L in MIN_SINGLE:
                    k = record([dst, "-l", lens_path, "-s", str(s), "-L", str(L)],
                               os.path.join(OUT, "%s.%s.s%d.L%d.bed" % (name, run, s, L)))
            print("%-13s %-6s %3d rows, %2d blocks, ends in a %s, %d lines at -s %d -L 0" %
                  (name, run, last + 1, len(blocks), "block" if blocks[-1, 1] == last else "free row", k, s))
    table = collmodel.make_table(**PARTIAL)
    src = os.path.join(OUT, "partial.mums")
    open(src, "wb").write(collmodel.mums_bytes(*table))
    lens_path = os.path.join(OUT, "partial.lengths")
    write_lengths(lens_path, "partial", contig_lengths("partial", table, None, rng))
    for s in (0, 1, table[1].shape[1] - 1):
        for L in MIN_SINGLE:
            k = record([src, "-l", lens_path, "-s", str(s), "-L", str(L), "-v"], os.path.join(OUT, "partial.s%d.L%d.bed" % (s, L)))
    print("%-13s no blocks, %d rows, %d lines at -s %d -L 0" % ("partial", len(table[0]), k, s))


if __name__ == "__main__":
    main()
