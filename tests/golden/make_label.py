#!/usr/bin/env python3
"""Golden fixtures of the contig labels.  Run HERE: needs the reference mounted at /root/reference (its
mumemto/get_sequence_info.py is imported from there, never copied); the fixtures are data only.

The reference package's __init__ imports a compiled core, so an empty module `mumemto` whose __path__ is the reference's
package directory is registered before the import: its pure-Python modules load, its __init__ never runs.

label/
  <table>.<run>.mums, <table>.lengths   the tables and contigs of make_bed.py's recipe, taken from tests/golden/bed: synteny,
                                        inversion, moved and minus_column (contigs of length 0, a contig boundary exactly on
                                        a start), each as the reference's collinear tool wrote it with -g 1000 and -g 0
  partial.mums, partial.lengths         a table without blocks and with absent cells
  <table>[.<run>].labeled.mums          written by the reference's get_sequence_info tool from them
  <table>[.<run>].named.mums            the same with -n

The reference itself finishes on every one of them: no start lies at or beyond its sequence's total, and no file carries `-` in
the block field of every row.
"""
import contextlib
import io
import os
import shutil
import sys
import types

pkg = types.ModuleType("mumemto")
pkg.__path__ = ["/root/reference/mumemto"]
sys.modules["mumemto"] = pkg
from mumemto import get_sequence_info as ref_label  # noqa: E402  (the reference's module; never copied)

HERE = os.path.dirname(os.path.abspath(__file__))
BED, OUT = os.path.join(HERE, "bed"), os.path.join(HERE, "label")
TABLES = [(name, "%s.%s" % (name, run)) for name in ("synteny", "inversion", "moved", "minus_column") for run in ("g1000", "g0")]
TABLES.append(("partial", "partial"))


def record(argv, dst):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        ref_label.main(ref_label.parse_arguments(argv + ["-o", dst]))
    return open(dst).read().count("\n")


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    for name, table in TABLES:
        src, lens = os.path.join(OUT, table + ".mums"), os.path.join(OUT, name + ".lengths")
        shutil.copyfile(os.path.join(BED, table + ".mums"), src)
        shutil.copyfile(os.path.join(BED, name + ".lengths"), lens)
        k = record(["-m", src, "-l", lens], os.path.join(OUT, table + ".labeled.mums"))
        assert k == record(["-m", src, "-l", lens, "-n"], os.path.join(OUT, table + ".named.mums"))
        print("%-20s %3d lines" % (table, k))


if __name__ == "__main__":
    main()
