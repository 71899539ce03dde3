"""`collinear` -- label every multi-MUM of a .mums / .bumbl file with the collinear block it belongs to.

Twin of the reference's `mumemto collinear` (mumemto/collinear_block.py on mumemto/utils.py find_coll_blocks), same flags and
defaults, same output bytes; the blocks are found on the GPU (csrc/collinear.cpp), and a .mums output is formatted there.

  python -m mumemto_amd.collinear_block -m run.mums                 -> run_sorted.mums
  python -m mumemto_amd.collinear_block -i run -o blocks.bumbl -g 0

Rows with an absent document are dropped and the rest is ordered by the first document before blocks are looked for, so
the output holds strict multi-MUMs only.  A fourth field already on the input (blocks of an earlier run) is replaced; a
file with a fifth field is refused.  Equal starts within one column are ordered by row.  There is no host fallback: without a
usable GPU the tool stops with the library's message.
"""
import argparse
import os
import sys

import numpy as np

from . import mumsio


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.collinear_block", description="Computes collinear blocks of MUMs")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input-prefix", "-i", dest="prefix", help="prefix of the .bumbl or .mums file (.bumbl wins)")
    src.add_argument("--mums", "-m", dest="mumfile", help="path to a .mums or .bumbl file")
    ap.add_argument("--fout", "-o", dest="filename", help="output file (default: input name + _sorted)")
    ap.add_argument("--max-gap-len", "-g", dest="max_break", type=int, default=1000,
                    help="maximum break between collinear MUMs within a block, 0 = no limit (default: 1000)")
    ap.add_argument("--verbose", "-v", dest="verbose", action="store_true", default=False, help="verbose mode")
    ap.add_argument("--min-singleton-length", dest="min_singleton_length", type=int, default=None,
                    help="minimum length of singleton blocks to include (default: no singletons)")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    args = ap.parse_args(argv)
    if args.mumfile is None:
        prefix = args.prefix
        if prefix.endswith((".mums", ".bumbl")):
            prefix = os.path.splitext(prefix)[0]
        for ext in (".bumbl", ".mums"):
            if os.path.exists(prefix + ext):
                args.mumfile = prefix + ext
                break
        else:
            ap.error("neither %s.bumbl nor %s.mums exists" % (prefix, prefix))
    if args.max_break < 0 or args.max_break > 0xFFFFFFFF:
        ap.error("--max-gap-len must lie in [0, 2^32)")
    if args.filename is None:
        stem, ext = os.path.splitext(args.mumfile)
        args.filename = stem + "_sorted" + ext
    if not args.filename.endswith((".mums", ".bumbl")):
        args.filename += ".mums"
    return args


def main(args):
    if not args.mumfile.endswith(".bumbl") and mumsio.mums_extra_fields(args.mumfile) > 4:
        print("Error: %s carries fields beyond the block field; extra fields are not supported." % args.mumfile,
              file=sys.stderr)
        return 1
    lengths, starts, strands = mumsio.read_rows(args.mumfile)
    if args.verbose:
        print("Found %d MUMs" % len(lengths), file=sys.stderr)
    if len(lengths) == 0 or (starts == -1).any(axis=1).all():
        print("No strict MUMs found after filtering partial MUMs.", file=sys.stderr)
        return 0
    if args.verbose:
        print("Finding collinear blocks (max gap = %s bp)..." % (args.max_break or None), file=sys.stderr)
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    try:
        with mumemto_amd.Merged.from_rows(eng, lengths, starts, strands) as m:
            blocks = m.collinear(args.max_break, args.min_singleton_length)
            if args.verbose:
                print("found %d collinear blocks" % len(blocks), file=sys.stderr)
            if args.filename.endswith(".mums"):
                m.write_text(args.filename)
            else:
                length, off, st = m.rows()
                mumsio.write_bumbl(args.filename, length.astype(np.uint32), off, st.astype(bool), blocks=blocks)
    finally:
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
