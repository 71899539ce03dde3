"""`extract_mums` -- the sequences of the multi-MUMs of a .mums / .bumbl table as a multi-FASTA.

Twin of the reference's Python tool (mumemto/extract_mums.py), same flags and defaults: record i is `>mum_<i>`, the bases of row i
in sequence -i, upper-cased, reverse-complemented when the row lies on `-` there, and a `#`; the records are joined by
newlines, with none after the last.  The bases are gathered and the bytes made on the GPU (csrc/sequences.cpp) from the whole
table at once, and the library writes the file (PATH.tmp, renamed).

  python -m mumemto_amd.extract_mums -m run.mums                 (FASTA paths from run.lengths, output run_mums.fa)
  python -m mumemto_amd.extract_mums -m run.bumbl -i 2 -o third

Decided where the reference leaves it open or to a library that is not here:
  1. The reference complements with Biopython.  Here: A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; W, S, N, X and every other
     byte stay (csrc/sequence_kernels.hip).
  2. A row that runs over the sequence's end is cut there; one that starts at or beyond it, or has no start in the sequence
     (-1), gives an empty record -- what Python's slice yields.
  3. Where the reference asserts -- the sequence's length differs from the lengths file's entry -- the tool prints the
     reference's message and exits 1, before anything is written.
  4. The FASTA file is read as the library reads every FASTA (records concatenated; gzip works).

Additions: -t/--no-terminator (no `#`), --dialect binary (the bytes of the reference's extract_mums BINARY: bases as they are,
strands ignored, a newline behind every record, rows without a start or starting beyond the end refused), --device.  There is
no host fallback: without a usable GPU the tool stops with the library's message.

Imported as a module, `mumemto_amd.extract_mums(lengths, starts, strands, source, ...)` stays callable: the call goes to
mumemto_amd.binding.extract_mums.
"""
import argparse
import os
import sys
import types

import numpy as np

from . import mumsio


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.extract_mums", description="Extract the MUM sequences")
    ap.add_argument("-m", "--mumfile", type=str, required=True, help="bumbl file to process")
    ap.add_argument("-i", "--index", type=int, default=0, help="The index of the file in the corresponding filelist")
    ap.add_argument("-o", "--output", type=str, help="The name of the output file")
    ap.add_argument("-f", "--filelist", type=str, help="filelist file")
    ap.add_argument("-v", "--verbose", action="store_true", help="Print verbose output")
    ap.add_argument("-t", "--no-terminator", dest="terminator", action="store_false",
                    help="do not add terminator (#) to end of each MUM sequence")
    ap.add_argument("--dialect", choices=("python", "binary"), default="python",
                    help="python: this tool's bytes (default); binary: those of the extract_mums binary")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    args = ap.parse_args(argv)
    if args.filelist is None:
        args.filelist = os.path.splitext(args.mumfile)[0] + ".lengths"
        if not os.path.exists(args.filelist):
            print("Filelist %s not found, and no filelist provided" % args.filelist, file=sys.stderr)
            sys.exit(1)
    if args.output is None:
        args.output = os.path.splitext(args.mumfile)[0] + "_mums.fa"
    if not args.output.endswith(".fa") and not args.output.endswith(".fasta"):
        args.output += ".fa"
    return args


def seq_paths(filelist):
    """the FASTA path of every sequence: the first token of every line, or of a multi-FASTA lengths file of its `PATH * total`
    lines (mumemto/utils.py:209-219)"""
    lines = [l.split() for l in open(filelist).read().splitlines()]
    if lines and len(lines[0]) > 1 and lines[0][1] == "*":
        return [l[0] for l in lines if l[1] == "*"]
    return [l[0] for l in lines]


def main(args):
    try:
        paths = seq_paths(args.filelist)
        seq_lengths = mumsio.read_seq_lengths(args.filelist)
    except (OSError, IndexError, ValueError) as ex:
        print("Error: cannot read the filelist %s: %s" % (args.filelist, ex), file=sys.stderr)
        return 1
    if not 0 <= args.index < len(paths):
        print("Error: index %d is out of range: %s lists %d sequences" % (args.index, args.filelist, len(paths)), file=sys.stderr)
        return 1
    fasta = paths[args.index]
    if not os.path.exists(fasta):
        print("File %s not found. Ensure lengths file is formatted correctly. Perhaps the paths are relative, not absolute?" % fasta,
              file=sys.stderr)
        return 1
    try:
        lengths, starts, strands = mumsio.read_rows(args.mumfile)
    except (OSError, ValueError, IndexError) as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    if not len(lengths):                                   # (a table without rows has no columns of its own)
        starts = np.zeros((0, len(paths)), np.int64)
        strands = np.zeros((0, len(paths)), bool)
    if starts.shape[1] != len(paths):
        print("Error: %s has %d sequences, %s lists %d" % (args.mumfile, starts.shape[1], args.filelist, len(paths)), file=sys.stderr)
        return 1
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    try:
        with mumemto_amd.Merged.from_rows(eng, lengths, starts, strands) as m:
            if args.verbose:
                print("Extracting MUMs", file=sys.stderr)
            n_bytes = m.sequences(args.index, fasta, args.dialect, args.terminator)
            if m.sequences_doc_bases != seq_lengths[args.index]:
                print("Sequence length %d does not match expected length %d. There may be Ns or other non-ACGT chars in the "
                      "FASTA file." % (m.sequences_doc_bases, seq_lengths[args.index]), file=sys.stderr)
                return 1
            m.write_sequences(args.output)
            if args.verbose:
                print("%d records, %d bytes to %s: %s" % (m.n_rows, n_bytes, args.output, m.sequences_stats()), file=sys.stderr)
    except mumemto_amd.MumemtoError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    finally:
        eng.close()
    return 0


class _CallableModule(types.ModuleType):
    """`import mumemto_amd.extract_mums` binds this module over the function of the same name in the package: calls go on"""

    def __call__(self, *args, **kwargs):
        from .binding import extract_mums
        return extract_mums(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
else:
    sys.modules[__name__].__class__ = _CallableModule
