"""`coverage` -- the share of a sequence that the multi-MUMs of a .mums / .bumbl file cover.

Twin of the reference's `mumemto coverage` (mumemto/mum_coverage.py), same flags and defaults, same bytes: one line
`seq<idx>: <percent, three decimals>%` on stderr, nothing on stdout.  The union of the intervals is formed on the GPU
(csrc/coverage.cpp) from the whole table at once; the percentage is formatted here from the integer the device returns.

  python -m mumemto_amd.mum_coverage -m run.mums -s 3                    (lengths from run.lengths)
  python -m mumemto_amd.mum_coverage -i run -L 200
  python -m mumemto_amd.mum_coverage -i run --all --runs run.covered.tsv

A row takes part when the sequence has a start in it and its length is at least -L; it covers [start, start + length), cut at
the end of the sequence.  Two additions: --all prints one line per sequence of the lengths file, in order, from one pass over
the table (the reference needs one invocation per sequence); --runs PATH writes the covered stretches themselves, one line
`seq<idx> <TAB> begin <TAB> end` (half-open) per maximal stretch of the sequences asked for, to PATH.tmp, renamed when complete.

One departure from the reference: a sequence index that the lengths file has but the table has no column for is refused with
a message (the reference raises IndexError).  There is no host fallback: without a usable GPU the tool stops with the
library's message.

Imported as a module, `mumemto_amd.mum_coverage(lengths, starts, strands, seq_lengths, ...)` stays callable: the call goes to
mumemto_amd.binding.mum_coverage.
"""
import argparse
import os
import sys
import types

import numpy as np

from . import mumsio


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.mum_coverage",
                                 description="Aggregates MUM coverage from mumemto output.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input-prefix", "-i", dest="prefix", help="prefix for filelist, mums, and lengths files")
    src.add_argument("--mums", "-m", dest="mumfile", help="path to a .mums or .bumbl file")
    ap.add_argument("--lengths", "-l", dest="lens", help="lengths file (default: PREFIX.lengths)")
    ap.add_argument("--len-filter", "-L", dest="lenfilter", default=0, type=int, help="only consider MUMs of at least this length")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--seq-idx", "-s", dest="seq_idx", type=int, help="sequence index to compute coverage for (default: 0)")
    which.add_argument("--all", dest="all", action="store_true", help="every sequence of the lengths file, one line each")
    ap.add_argument("--runs", dest="runs", metavar="PATH", help="write the covered stretches: seq<idx>, begin, end (half-open)")
    ap.add_argument("--verbose", "-v", dest="verbose", action="store_true", help="verbose mode")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    args = ap.parse_args(argv)
    if args.seq_idx is None:
        args.seq_idx = 0
    if args.mumfile:
        args.prefix = os.path.splitext(args.mumfile)[0]
    else:
        bumbl, mums = os.path.exists(args.prefix + ".bumbl"), os.path.exists(args.prefix + ".mums")
        if bumbl and mums:
            print("Error: Both %s and %s exist. Please specify the file explicitly with --mums."
                  % (args.prefix + ".bumbl", args.prefix + ".mums"), file=sys.stderr)
            sys.exit(1)
        elif bumbl:
            args.mumfile = args.prefix + ".bumbl"
        elif mums:
            args.mumfile = args.prefix + ".mums"
        elif args.prefix.endswith((".bumbl", ".mums")):
            args.mumfile = args.prefix
            args.prefix = os.path.splitext(args.prefix)[0]
        else:
            args.mumfile = args.prefix + ".mums"
    if args.lens is None:
        args.lens = args.prefix + ".lengths"
    return args


def format_coverage(idx, covered, seq_length):
    """the reference's line: Python's true division of two ints, three decimals"""
    return "seq%d: %.3f%%" % (idx, int(covered) * 100 / int(seq_length))


def write_runs(path, columns, run_begin, runs):
    with open(path + ".tmp", "w") as f:
        for c in columns:
            for b, e in runs[int(run_begin[c]):int(run_begin[c + 1])].tolist():
                f.write("seq%d\t%d\t%d\n" % (c, b, e))
    os.replace(path + ".tmp", path)


def main(args):
    try:
        seq_lengths = mumsio.read_seq_lengths(args.lens)
    except (OSError, ValueError, IndexError) as ex:
        print("Error: cannot read the lengths file %s: %s" % (args.lens, ex), file=sys.stderr)
        return 1
    if args.seq_idx >= len(seq_lengths) or args.seq_idx < 0:
        print("Error: sequence index %d is out of range (0-%d)" % (args.seq_idx, len(seq_lengths) - 1), file=sys.stderr)
        return 1
    if not args.mumfile.endswith((".mums", ".bumbl")):
        print("Error: %s does not end with .mums or .bumbl" % args.mumfile, file=sys.stderr)
        return 1
    if args.verbose:
        print("Reading %s..." % args.mumfile, file=sys.stderr)
    try:
        lengths, starts, strands = mumsio.read_rows(args.mumfile)
    except OSError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    if not len(lengths):                                   # (a table without rows has no columns of its own)
        starts = np.zeros((0, len(seq_lengths)), np.int64)
        strands = np.zeros((0, len(seq_lengths)), bool)
    n_docs = starts.shape[1]
    columns = list(range(len(seq_lengths))) if args.all else [args.seq_idx]
    if columns[-1] >= n_docs:
        print("Error: sequence index %d is beyond the %d sequences of %s" % (columns[-1], n_docs, args.mumfile), file=sys.stderr)
        return 1
    # the library wants a length per column; those not asked for (a lengths file shorter than the table) are not looked at
    lens = np.ones(n_docs, np.int64)
    k = min(n_docs, len(seq_lengths))
    lens[:k] = seq_lengths[:k]
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    try:
        with mumemto_amd.Merged.from_rows(eng, lengths, starts, strands) as m:
            if args.verbose:
                print("Computing coverage of %d rows x %d sequences..." % (len(lengths), n_docs), file=sys.stderr)
            covered = m.coverage(lens, None if args.all else args.seq_idx, args.lenfilter)
            run_begin, runs = m.coverage_runs() if args.runs else (None, None)
    except mumemto_amd.MumemtoError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    finally:
        eng.close()
    if args.runs:
        try:
            write_runs(args.runs, columns, run_begin, runs)
        except OSError as ex:
            print("Error: %s" % ex, file=sys.stderr)
            return 1
    for c in columns:
        print(format_coverage(c, covered[c], seq_lengths[c]), file=sys.stderr)
    return 0


class _CallableModule(types.ModuleType):
    """`import mumemto_amd.mum_coverage` binds this module over the function of the same name in the package: calls go on"""

    def __call__(self, *args, **kwargs):
        from .binding import mum_coverage
        return mum_coverage(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
else:
    sys.modules[__name__].__class__ = _CallableModule
