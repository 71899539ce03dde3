"""`label` -- a .mums / .bumbl table with every start also given as (contig, offset inside that contig).

Twin of the reference's `mumemto label` (mumemto/get_sequence_info.py), same flags and defaults, same bytes: one line

  LEN <TAB> s_0,...,s_{N-1} <TAB> +|-,... <TAB> BLOCK <TAB> c_0,...,c_{N-1} <TAB> rel_0,...,rel_{N-1}

per row, in the order of the file, nothing filtered.  c_j is the contig (FASTA record) of sequence j that holds the start, among
those the multi-FASTA lengths file lists, rel_j the start inside that contig; with -n c_j is the contig's name.  An absent
start is printed as -1 in fields 2 and 6 and gets contig 0.  BLOCK is `*` for a file without collinear blocks, else the row's
block or `-`.  The lookup and the bytes are made on the GPU (csrc/label.cpp) from the whole table at once, and the library
writes the file (PATH.tmp, renamed).

  python -m mumemto_amd.get_sequence_info -m run.mums                    (lengths from run.lengths, output run_labeled.mums)
  python -m mumemto_amd.get_sequence_info -m run -n -o run.named.mums

Three departures from the reference, all decided:
  1. A start at or beyond the total length of its sequence stops the tool with a message that names the first such row and
     column (the reference raises IndexError); a silently clamped label would be worse than none.
  2. A .mums file whose block field is `-` on every row gets `-` on every row (the reference crashes on its empty block list).
  3. The blocks of a file are attached as `mumemto collinear` leaves them: rows without absent starts, ascending in sequence
     0.  A file that breaks either stops the tool with the library's message.

Addition: --device.  There is no host fallback: without a usable GPU the tool stops with the library's message.

Imported as a module, `mumemto_amd.get_sequence_info(lengths, starts, strands, contigs, ...)` stays callable: the call goes to
mumemto_amd.binding.get_sequence_info.
"""
import argparse
import os
import sys
import types

import numpy as np

from . import mumsio
from .find_inversions import blocks_of_rows


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.get_sequence_info", description="Extract the MUM sequences")
    ap.add_argument("-m", "--mumfile", required=True, help="path to the .mums or .bumbl file (or its prefix)")
    ap.add_argument("-o", "--output", help="path to the output file (default: the MUMs file's name with _labeled.mums)")
    ap.add_argument("-l", "--lengths", help="multi-FASTA lengths file (default: the MUMs file's name with .lengths)")
    ap.add_argument("-v", "--verbose", action="store_true", help="progress on stderr (never changes the output)")
    ap.add_argument("-n", "--contig-names", dest="contig_names", action="store_true",
                    help="print contig names/sequence IDs instead of numerical indexes")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    args = ap.parse_args(argv)
    if not args.mumfile.endswith((".mums", ".bumbl")):
        if os.path.exists(args.mumfile + ".mums"):
            args.mumfile += ".mums"
        elif os.path.exists(args.mumfile + ".bumbl"):
            args.mumfile += ".bumbl"
        else:
            print("MUM file %s not found." % args.mumfile, file=sys.stderr)
            sys.exit(1)
    elif not os.path.exists(args.mumfile):
        print("MUM file %s not found." % args.mumfile, file=sys.stderr)
        sys.exit(1)
    if args.lengths is None:
        args.lengths = os.path.splitext(args.mumfile)[0] + ".lengths"
    if not os.path.exists(args.lengths):
        print("Lengths file %s not found." % args.lengths, file=sys.stderr)
        sys.exit(1)
    if args.output is None:
        args.output = os.path.splitext(args.mumfile)[0] + "_labeled.mums"
    return args


def main(args):
    try:
        contigs = mumsio.read_contigs(args.lengths)
    except ValueError:
        print("Multi-FASTA input required for contig ID annotation.", file=sys.stderr)
        return 1
    except (OSError, IndexError) as ex:
        print("Error: cannot read the lengths file %s: %s" % (args.lengths, ex), file=sys.stderr)
        return 1
    try:
        if args.mumfile.endswith(".bumbl"):
            lengths, starts, strands, blocks = mumsio.read_bumbl(args.mumfile, with_blocks=True)
        else:
            lengths, starts, strands, row_block = mumsio.read_mums(args.mumfile, with_blocks=True)
            blocks = None if row_block is None else blocks_of_rows(row_block)
    except (OSError, ValueError) as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    n_seqs = len(contigs[0])
    if not len(lengths):                                   # (a table without rows has no columns of its own)
        starts = np.zeros((0, n_seqs), np.int64)
        strands = np.zeros((0, n_seqs), bool)
    if starts.shape[1] != n_seqs:
        print("Error: %s has %d sequences, %s lists %d" % (args.mumfile, starts.shape[1], args.lengths, n_seqs), file=sys.stderr)
        return 1
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    try:
        with mumemto_amd.Merged.from_rows(eng, lengths, starts, strands) as m:
            if blocks is not None:
                if args.verbose:
                    print("Using the collinear blocks of the file: %d blocks" % len(blocks), file=sys.stderr)
                m.set_blocks(blocks)
            if args.verbose:
                print("Transforming MUMs to contig-relative coordinates...", file=sys.stderr)
            n_bytes = m.label(contigs, args.contig_names)
            m.write_label(args.output)
            if args.verbose:
                print("%d rows x %d sequences, %d bytes to %s" % (m.n_rows, n_seqs, n_bytes, args.output), file=sys.stderr)
    except mumemto_amd.MumemtoError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    finally:
        eng.close()
    return 0


class _CallableModule(types.ModuleType):
    """`import mumemto_amd.get_sequence_info` binds this module over the function of the same name in the package: calls go on"""

    def __call__(self, *args, **kwargs):
        from .binding import get_sequence_info
        return get_sequence_info(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
else:
    sys.modules[__name__].__class__ = _CallableModule
