"""`bed` -- the collinear blocks and the long multi-MUMs of a .mums / .bumbl file as BED intervals of one sequence.

Twin of the reference's `mumemto bed` (mumemto/mum_to_bed.py), same flags and defaults, same bytes: one line
`contig <TAB> start <TAB> end <TAB> block_<b> | mum_<i> <TAB> + | -` per record, in the coordinates of the contigs (FASTA
records) that the multi-FASTA lengths file lists for the sequence.  Records, intervals, the contig lookup and the bytes are
made on the GPU (csrc/bed.cpp) from the whole table at once; with -o the library writes the file (PATH.tmp, renamed).

  python -m mumemto_amd.mum_to_bed run.mums -s 3 -o run.3.bed            (lengths from run.lengths)
  python -m mumemto_amd.mum_to_bed run.bumbl --all -o run                (run.<idx>.bed for every sequence, one pass)

A file with blocks (the fourth field `mumemto collinear` writes, or the block list of a .bumbl) gives one record per block,
[start of its first row, end of its last row) read along the strand of its last row, and one record `mum_<i>` per row in no
block that is at least -L long.  A file without blocks gives one `mum_<i>` per row of at least -L with a start in the
sequence; -g N computes the blocks first (max gap N, 0 = no limit), as `find_inversions` does.  i counts the rows that have
a start in the sequence.  The contig is the first one whose cumulative length exceeds the interval's start; an interval that
runs over its contig's end is not split.

Four departures from the reference, all decided:
  1. A block that ends the table is written (the reference never flushes its last block: the line is missing there).
  2. A block of one row (`collinear --min-singleton-length`) gives [start, start + length) (the reference leaves one end stale
     or None, and crashes when it is the first block).
  3. A file without blocks gives its `mum_<i>` lines with or without -v (the reference writes nothing without -v); -v never
     changes the output here.
  4. A start at or beyond the total length of the sequence gets the last contig (the reference raises IndexError); the number
     of such records is reported on stderr and in the library's statistics.

Additions: --all, -g, --device.  There is no host fallback: without a usable GPU the tool stops with the library's message.

Imported as a module, `mumemto_amd.mum_to_bed(lengths, starts, strands, contigs, ...)` stays callable: the call goes to
mumemto_amd.binding.mum_to_bed.
"""
import argparse
import os
import sys
import types

import numpy as np

from . import mumsio
from .find_inversions import blocks_of_rows


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.mum_to_bed", description="Convert MUMs file to BED file")
    ap.add_argument("mums_file", help="path to the .mums or .bumbl file")
    ap.add_argument("--lengths-file", "-l", help="multi-FASTA lengths file (default: the MUMs file's name with .lengths)")
    ap.add_argument("-v", "--verbose", action="store_true", help="progress on stderr (never changes the output)")
    ap.add_argument("--min-singleton-length", "-L", type=int, default=100, help="minimum length of a row outside every block")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--seq-idx", "-s", type=int, default=None, help="sequence to output BED coordinates for (default: 0)")
    which.add_argument("--all", dest="all", action="store_true", help="every sequence: OUTPUT.<idx>.bed each, from one pass")
    ap.add_argument("--output", "-o", default=None, help="output file (default: stdout); with --all the prefix of the files")
    ap.add_argument("--max-block-gap", "-g", type=int, default=None, metavar="N",
                    help="compute the collinear blocks of a file without blocks first (max gap N, 0 = no limit)")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    args = ap.parse_args(argv)
    if args.all and args.output is None:
        ap.error("--all needs -o PREFIX: the sequences go to PREFIX.<idx>.bed")
    if args.max_block_gap is not None and not 0 <= args.max_block_gap <= 0xFFFFFFFF:
        ap.error("--max-block-gap must lie in [0, 2^32)")
    if args.seq_idx is None:
        args.seq_idx = 0
    if args.lengths_file is None:
        args.lengths_file = os.path.splitext(args.mums_file)[0] + ".lengths"
    return args


def main(args):
    if not args.mums_file.endswith((".mums", ".bumbl")):
        print("Error: %s does not end with .mums or .bumbl" % args.mums_file, file=sys.stderr)
        return 1
    try:
        contigs = mumsio.read_contigs(args.lengths_file)
    except (OSError, ValueError, IndexError) as ex:
        print("Error: cannot read the lengths file %s: %s" % (args.lengths_file, ex), file=sys.stderr)
        return 1
    n_seqs = len(contigs[0])
    if args.seq_idx >= n_seqs or args.seq_idx < 0:
        print("Sequence index %d too large for dataset with %d sequences." % (args.seq_idx, n_seqs), file=sys.stderr)
        return 1
    try:
        if args.mums_file.endswith(".bumbl"):
            lengths, starts, strands, blocks = mumsio.read_bumbl(args.mums_file, with_blocks=True)
        else:
            lengths, starts, strands, row_block = mumsio.read_mums(args.mums_file, with_blocks=True)
            blocks = None if row_block is None else blocks_of_rows(row_block)
    except (OSError, ValueError) as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    if not len(lengths):                                   # (a table without rows has no columns of its own)
        starts = np.zeros((0, n_seqs), np.int64)
        strands = np.zeros((0, n_seqs), bool)
    n_docs = starts.shape[1]
    columns = list(range(n_seqs)) if args.all else [args.seq_idx]
    if columns[-1] >= n_docs:
        print("Error: sequence index %d is beyond the %d sequences of %s" % (columns[-1], n_docs, args.mums_file), file=sys.stderr)
        return 1
    # the library wants the contigs of every column; those not asked for (a lengths file shorter than the table) get none
    names = list(contigs[0][:n_docs]) + [[]] * (n_docs - min(n_docs, n_seqs))
    lens = list(contigs[1][:n_docs]) + [[]] * (n_docs - min(n_docs, n_seqs))
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    text = b""
    try:
        with mumemto_amd.Merged.from_rows(eng, lengths, starts, strands) as m:
            if blocks is not None:
                if args.verbose:
                    print("Using the collinear blocks of the file: %d blocks" % len(blocks), file=sys.stderr)
                m.set_blocks(blocks)
            elif args.max_block_gap is not None:
                if args.verbose:
                    print("Finding collinear blocks (max gap = %s bp)..." % (args.max_block_gap or None), file=sys.stderr)
                m.collinear(args.max_block_gap, None)
            elif args.verbose:
                print("No collinear blocks found. Only writing mums to BED intervals.", file=sys.stderr)
            n_records = m.bed((names, lens), None if args.all else args.seq_idx, args.min_singleton_length)
            if args.verbose:
                print("%d BED records of %d rows x %d sequences" % (n_records, m.n_rows, n_docs), file=sys.stderr)
            clamped = m.bed_stats()["clamped"]
            if clamped:
                print("Warning: %d records start at or beyond the end of their sequence in %s; they are given its last contig"
                      % (clamped, args.lengths_file), file=sys.stderr)
            if args.output is None:
                text = m.bed_text(args.seq_idx)
            elif args.all:
                for c in columns:
                    m.write_bed(c, "%s.%d.bed" % (args.output, c))
            else:
                m.write_bed(args.seq_idx, args.output)
    except mumemto_amd.MumemtoError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    finally:
        eng.close()
    if args.output is None:
        try:
            sys.stdout.buffer.write(text)
            sys.stdout.flush()
        except BrokenPipeError:
            os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())
    return 0


class _CallableModule(types.ModuleType):
    """`import mumemto_amd.mum_to_bed` binds this module over the function of the same name in the package: calls go on"""

    def __call__(self, *args, **kwargs):
        from .binding import mum_to_bed
        return mum_to_bed(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
else:
    sys.modules[__name__].__class__ = _CallableModule
