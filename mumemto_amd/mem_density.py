"""`mem_density` -- how many multi-MEM occurrences cover each position of each sequence of a .mems file.

Twin of the reference's mumemto/mem_density.py, same flags, same file: `<stem>_coverage.npy` beside the .mems file, float64 of
shape (number of sequences, longest sequence), value for value what the reference saves.  The rows go to the GPU in batches
(mumsio.read_mems), the depths are accumulated and summed there (csrc/density.cpp); neither `numba` nor `tqdm` is needed.

  python -m mumemto_amd.mem_density -m run.mems -l run.lengths
  python -m mumemto_amd.mem_density -m run.mems -l run.lengths --bin 1000 -o run.density.npy

An occurrence (doc, start) of a row of length l adds 1 to the positions of doc that numpy's slice start : start + l selects
on an axis as long as the longest sequence: the cut is at that length, not at the sequence's own, and a negative start wraps as
numpy wraps it.  With -v, occurrences with a negative start are reported in one warning line.  Two additions: --bin W sums the
depths over bins of W positions, shape (number of sequences, ceil(longest / W)) -- the per-base array of 94 human genomes
would be 2.3 TB, bins of 1000 make it 2.3 GB; -o PATH names the output.  The file is written as PATH.tmp and renamed when complete.

Two departures from the reference: a line whose starts and documents differ in count is refused with its line number (the
reference drops the tail of the longer field), and a document index that the lengths file has no sequence for is refused
with the row at fault (the reference raises IndexError).  There is no host fallback: without a usable GPU the tool stops
with the library's message.

Imported as a module, `mumemto_amd.mem_density(lengths, occ_start, starts, docs, seq_lengths, ...)` stays callable: the call
goes to mumemto_amd.binding.mem_density.
"""
import argparse
import os
import sys
import types

import numpy as np

from . import mumsio


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.mem_density",
                                 description="Aggregates MEM density for downstream plotting")
    ap.add_argument("--mems", "-m", dest="mems", help="path to mems from mumemto", required=True)
    ap.add_argument("--lengths", "-l", dest="lengths", help="lengths of each sequence", required=True)
    ap.add_argument("--verbose", "-v", dest="verbose", action="store_true", help="enable verbose mode")
    ap.add_argument("--bin", dest="bin", type=int, default=1, metavar="W", help="sum the depths over bins of W positions (default: 1)")
    ap.add_argument("--output", "-o", dest="output", metavar="PATH", help="output file (default: <stem of the .mems file>_coverage.npy)")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    ap.add_argument("--max-occ", dest="max_occ", type=int, default=1 << 24, help=argparse.SUPPRESS)      # occurrences per batch
    return ap.parse_args(argv)


def save(path, table):
    """np.save of the table, to PATH.tmp, renamed when complete"""
    with open(path + ".tmp", "wb") as f:
        np.save(f, table)
    os.replace(path + ".tmp", path)


def main(args):
    try:
        seq_lengths = mumsio.read_seq_lengths(args.lengths)
    except (OSError, ValueError, IndexError) as ex:
        print("Error: cannot read the lengths file %s: %s" % (args.lengths, ex), file=sys.stderr)
        return 1
    if args.bin < 1:
        print("Error: --bin must be 1 or more", file=sys.stderr)
        return 1
    out_path = args.output or os.path.splitext(args.mems)[0] + "_coverage.npy"
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    try:
        with mumemto_amd.Density(eng, seq_lengths, args.bin) as d:
            if args.verbose:
                print("Parsing %s..." % args.mems, file=sys.stderr)
            for batch in mumsio.read_mems(args.mems, args.max_occ):
                d.add_rows(*batch)
            d.finish()
            table = d.bins().astype(np.float64)
            st = d.stats()
    except (mumemto_amd.MumemtoError, OSError, ValueError) as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    finally:
        eng.close()
    if args.verbose and st["negative"]:
        print("Warning: %d of %d occurrences have a negative start; they wrap around the end as numpy's slices do"
              % (st["negative"], st["occurrences"]), file=sys.stderr)
    try:
        save(out_path, table)
    except OSError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    if args.verbose:
        print("Wrote %s: %d x %d, %d occurrences in %.3f ms on the device" % (out_path, table.shape[0], table.shape[1],
                                                                          st["occurrences"], st["add_ms"] + st["finish_ms"]),
              file=sys.stderr)
    return 0


class _CallableModule(types.ModuleType):
    """`import mumemto_amd.mem_density` binds this module over the function of the same name in the package: calls go on"""

    def __call__(self, *args, **kwargs):
        from .binding import mem_density
        return mem_density(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
else:
    sys.modules[__name__].__class__ = _CallableModule
