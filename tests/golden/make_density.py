#!/usr/bin/env python3
"""Golden fixtures of the MEM density.  Run HERE: needs the reference mounted at /root/reference (its mumemto/mem_density.py is
imported from there, never copied); the fixtures are data only.

The reference package's __init__ imports a compiled core, so an empty module `mumemto` whose __path__ is the reference's
package directory is registered before the import, as make_bed.py does.  The tool also wants `numba` and `tqdm`: two empty
modules stand in for them (`njit` returns its argument, `tqdm` returns its iterable), so that what is recorded is numpy's own
slice arithmetic, `coverage[idx, start:start+l] += 1`.

density/
  <name>.mems             hand-made (or seeded) MEM rows: length <TAB> starts <TAB> documents <TAB> strands
  <name>.lengths          the lengths file
  <name>_coverage.npy     what the reference's tool saved for them: float64 (num, max length)

  wraps       size 100: start -30, l 25 covers [70, 95); start -1, l 30 covers nothing; start 95, l 20 covers [95, 100);
              starts below -size (-120, l 150 covers [0, 30); -250, l 40 covers nothing); a negative start whose slice is whole
  edges       size 1000: start == size; start + l == size; start + l == size + 1; l covering the whole axis; pile-ups
  short_seq   lengths 300, 120, 50: the two short sequences are covered beyond their own ends, up to 300
  multifasta  a multi-FASTA lengths file (five sequences, 2 - 4 contigs each) and seeded rows (tests/densmodel.py make_rows)
"""
import os
import shutil
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = types.ModuleType("mumemto")
pkg.__path__ = ["/root/reference/mumemto"]
sys.modules["mumemto"] = pkg
numba = types.ModuleType("numba")
numba.njit = lambda f: f
sys.modules["numba"] = numba
tqdm = types.ModuleType("tqdm")
tqdm_auto = types.ModuleType("tqdm.auto")
tqdm_auto.tqdm = tqdm.tqdm = lambda it, **kw: it
tqdm.auto = tqdm_auto
sys.modules["tqdm"] = tqdm
sys.modules["tqdm.auto"] = tqdm_auto
import numpy as np  # noqa: E402
import densmodel  # noqa: E402
from mumemto import mem_density as ref_density  # noqa: E402  (the reference's module; never copied)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "density")

# (length, [(document, start), ...]) per row
HAND = {
    "wraps": ([100, 100], [
        (25, [(0, -30), (1, 10)]),
        (30, [(0, -1), (1, -1), (1, 50)]),
        (20, [(0, 95), (1, 95)]),
        (150, [(0, -120), (1, -120)]),
        (40, [(0, -250), (1, -101)]),
        (100, [(0, -100), (1, -100), (1, 0)]),
    ]),
    "edges": ([1000, 640, 1000], [
        (17, [(0, 1000), (1, 1000), (2, 983)]),
        (64, [(0, 936), (1, 936), (2, 937)]),
        (1000, [(0, 0), (2, 0)]),
        (2000, [(1, 0), (2, 1)]),
        (1, [(0, 0), (0, 999), (2, 999), (2, 1000)]),
        (33, [(1, 500)] * 7 + [(2, 500)] * 70),
    ]),
    "short_seq": ([300, 120, 50], [
        (60, [(0, 200), (1, 100), (2, 40)]),
        (90, [(1, 200), (2, 200), (2, 250)]),
        (10, [(1, 119), (1, 120), (2, 49), (2, 50), (2, 299)]),
    ]),
}


def write_hand(name, seq_lengths, rows):
    with open(os.path.join(OUT, name + ".lengths"), "w") as f:
        for c, v in enumerate(seq_lengths):
            f.write("/data/genomes/%s_%d.fa %d\n" % (name, c, v))
    with open(os.path.join(OUT, name + ".mems"), "w") as f:
        for length, occ in rows:
            f.write("%d\t%s\t%s\t%s\n" % (length, ",".join(str(s) for _, s in occ), ",".join(str(d) for d, _ in occ),
                                          ",".join("+-"[i & 1] for i in range(len(occ)))))


def write_multifasta(name):
    rng = np.random.default_rng(11)
    totals = [1500, 1390, 1500, 700, 1213]
    with open(os.path.join(OUT, name + ".lengths"), "w") as f:
        for c, total in enumerate(totals):
            k = int(rng.integers(2, 5))
            cuts = np.sort(rng.choice(np.arange(1, total), k - 1, replace=False))
            fasta = "/data/genomes/%s_%d.fa" % (name, c)
            f.write("%s * %d\n" % (fasta, total))
            for j, v in enumerate(np.diff(np.concatenate(([0], cuts, [total]))).tolist()):
                f.write("%s %s_%d_ctg%d %d\n" % (fasta, name, c, j, v))
    rows = densmodel.make_rows(seed=12, n_rows=40, num=len(totals), size=max(totals), max_len=400)
    open(os.path.join(OUT, name + ".mems"), "wb").write(densmodel.mems_bytes(*rows, strands=np.arange(len(rows[2])) % 3 == 0))


def record(name):
    mems, lens = os.path.join(OUT, name + ".mems"), os.path.join(OUT, name + ".lengths")
    ref_density.main(types.SimpleNamespace(mems=mems, lengths=lens, verbose=False))     # (the tool rebinds args.lengths)
    cov = np.load(os.path.join(OUT, name + "_coverage.npy"))
    print("%-11s %s %s, sum %d, max %d, %d bytes" % (name, cov.dtype, cov.shape, cov.sum(), cov.max(),
                                                     os.path.getsize(os.path.join(OUT, name + "_coverage.npy"))))
    # (the model must already agree with what was recorded, or the fixtures would pin a misunderstanding)
    assert np.array_equal(cov, densmodel.loop(*densmodel.read_mems_plain(mems), densmodel.sequence_lengths(lens))), name
    return cov


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for name, (seq_lengths, rows) in HAND.items():
        write_hand(name, seq_lengths, rows)
        record(name)
    write_multifasta("multifasta")
    record("multifasta")


if __name__ == "__main__":
    main()
