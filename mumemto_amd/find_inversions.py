"""`inversion` -- call inversions from the collinear blocks of the multi-MUMs of a .mums / .bumbl file.

Twin of the reference's `mumemto inversion` (mumemto/find_inversions.py), same flags and defaults, same bytes on stdout; the
blocks and the calls are found on the GPU (csrc/collinear.cpp, csrc/inversion.cpp).

  python -m mumemto_amd.find_inversions -m run.mums                       (names from run.lengths)
  python -m mumemto_amd.find_inversions -i run -g 0 -L 500000
  python -m mumemto_amd.find_inversions -i run -a agp_files.txt -c 7 -d 0.05

One line per call: hap_id, start and end in that haplotype, ref_start and ref_end in the first sequence.  A call is a stretch
of at least two collinear blocks that lie on '-' in the haplotype and follow each other in reverse; a single reversed block
is not reported.  An input that carries blocks (a .bumbl written by `collinear_block`, or the fourth field of a .mums file)
whose rows are in order is taken with those blocks; otherwise rows with an absent document are dropped, the rest is ordered
by the first document and the blocks are computed with -g.  With -a and -c two columns follow: whether a scaffold break of
the haplotype's AGP file (component lines, `W`, of chr<C>) lies within margin x (end - start) of the start or of the end,
and the names of those components, start side first, or NA.

Departures from the reference: pre-computed blocks over a table with a partial row are refused (the reference computes on -1
starts); lines of the AGP list beyond the last sequence are ignored (the reference raises IndexError); a haplotype whose AGP
file has no `W` line of the chromosome gets `False`, `NA` (the reference raises on an empty minimum).  Equal starts within one
column are ordered by row.  There is no host fallback: without a usable GPU the tool stops with the library's message.

Imported as a module, `mumemto_amd.find_inversions(lengths, starts, strands, ...)` stays callable: the call goes to
mumemto_amd.binding.find_inversions.
"""
import argparse
import os
import sys
import types

import numpy as np

from . import mumsio

HEADER = "hap_id\tstart\tend\tref_start\tref_end"


def parse_arguments(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mumemto_amd.find_inversions",
                                 description="Detect inversions from MUMs. Optionally checks if inversions are flanked by "
                                             "scaffold breaks when AGP files are provided.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input-prefix", "-i", dest="prefix", help="prefix of the .bumbl or .mums file (.bumbl wins) and the lengths file")
    src.add_argument("--mums", "-m", dest="mumfile", help="path to a .mums or .bumbl file")
    ap.add_argument("--agp-filelist", "-a", dest="agp_filelist",
                    help="file with one AGP path per line, in the order of the sequences behind the first (the reference)")
    ap.add_argument("--filelist", "-f", dest="filelist", help="file with the sequence names (default: PREFIX.lengths)")
    ap.add_argument("--chr", "-c", help="chromosome number (required with --agp-filelist)")
    ap.add_argument("--margin", "-d", dest="margin", type=float, default=0.01,
                    help="proximity margin of a scaffold break, as a fraction of the inversion's length (default: 0.01)")
    ap.add_argument("--max-length", "-L", dest="max_length", type=int, help="maximum inversion length to report")
    ap.add_argument("--max-block-gap-len", "-g", dest="max_block_gap", type=int, default=1000,
                    help="maximum break between collinear MUMs within a block, 0 = no limit (default: 1000)")
    ap.add_argument("--verbose", "-v", action="store_true", help="print progress updates")
    ap.add_argument("--device", type=int, default=int(os.environ.get("MUMEMTO_DEVICE", "0")), help="GPU to use (default: 0)")
    args = ap.parse_args(argv)
    if bool(args.agp_filelist) ^ bool(args.chr):
        ap.error("--agp-filelist and --chr must be provided together")
    args.scaffold = bool(args.agp_filelist)
    if args.mumfile:
        args.prefix = os.path.splitext(args.mumfile)[0]
    else:
        if args.prefix.endswith((".mums", ".bumbl")):
            args.prefix = os.path.splitext(args.prefix)[0]
        for ext in (".bumbl", ".mums"):
            if os.path.exists(args.prefix + ext):
                args.mumfile = args.prefix + ext
                break
        else:
            ap.error("No .mums or .bumbl file found for prefix")
    if args.max_block_gap < 0 or args.max_block_gap > 0xFFFFFFFF:
        ap.error("--max-block-gap-len must lie in [0, 2^32)")
    if args.filelist is None:
        args.filelist = args.prefix + ".lengths"
    return args


def sequence_names(path, chrom=None):
    """the first field of every line of a lengths file (of a multi-FASTA one: of its `*` lines), as a base name, cut at
    _chr<C> when a chromosome is given"""
    lines = [l.split() for l in open(path).read().splitlines()]
    if lines and len(lines[0]) > 1 and lines[0][1] == "*":
        lines = [l for l in lines if l[1] == "*"]
    names = [os.path.basename(l[0]) for l in lines]
    return [n.split("_chr%s" % chrom)[0] for n in names] if chrom else names


def scaffold_breaks(agp_filelist, chrom, hap_ids, verbose=False):
    """-> {hap_id: (break positions, component names)}: line k of the list belongs to sequence k + 1"""
    agp_files = {}
    with open(agp_filelist) as f:
        for k, line in enumerate(f):
            if k + 1 >= len(hap_ids):
                break
            if line.strip():
                agp_files[hap_ids[k + 1]] = line.strip()
    out = {}
    for hap in hap_ids[1:]:
        path = agp_files.get(hap)
        if path is None:
            continue
        if not os.path.exists(path):
            if verbose:
                print("Warning: AGP file not found: %s" % path, file=sys.stderr)
            continue
        rows = [l.split() for l in open(path).read().splitlines() if l.startswith("chr" + str(chrom))]
        rows = [r for r in rows if r[4] == "W"]
        ends, at = [], 0
        for r in rows:
            at += int(r[2]) - int(r[1]) + 1
            ends.append(at)
        out[hap] = (ends, [r[5] for r in rows])
    return out


def format_calls(calls, hap_ids, breaks=None, margin=0.01):
    """the bytes of stdout: header and one line per call (breaks: scaffold_breaks(), or None without -a / -c)"""
    lines = [HEADER + ("\tscaffold_break\tcontig" if breaks is not None else "")]
    for col, start, end, ref_start, ref_end in np.asarray(calls, np.int64).reshape(-1, 5).tolist():
        hap = hap_ids[col]
        line = "%s\t%d\t%d\t%d\t%d" % (hap, start, end, ref_start, ref_end)
        if breaks is not None and hap in breaks:
            ends, names = breaks[hap]
            near = (end - start) * margin
            hit = [names[k] for k, p in enumerate(ends) if abs(p - start) < near]
            hit += [names[k] for k, p in enumerate(ends) if abs(p - end) < near]
            line += "\t%s\t%s" % (bool(hit), ",".join(hit) if hit else "NA")
        lines.append(line)
    return "".join(l + "\n" for l in lines)


def blocks_of_rows(row_block):
    """the fourth field of a .mums file -> (n_blocks, 2): maximal stretches of rows with the same block number"""
    rb = np.asarray(row_block, np.int64)
    if not len(rb):
        return np.zeros((0, 2), np.uint32)
    cut = np.nonzero(np.diff(rb) != 0)[0] + 1
    first = np.concatenate(([0], cut))
    last = np.concatenate((cut - 1, [len(rb) - 1]))
    keep = rb[first] != mumsio.NO_BLOCK
    return np.stack([first[keep], last[keep]], axis=1).astype(np.uint32)


def main(args):
    if args.verbose:
        print("Loading sequence information...", file=sys.stderr)
    try:
        hap_ids = sequence_names(args.filelist, args.chr)
        breaks = scaffold_breaks(args.agp_filelist, args.chr, hap_ids, args.verbose) if args.scaffold else None
    except OSError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    if args.mumfile.endswith(".bumbl"):
        lengths, starts, strands, blocks = mumsio.read_bumbl(args.mumfile, with_blocks=True)
    else:
        lengths, starts, strands, row_block = mumsio.read_mums(args.mumfile, with_blocks=True)
        blocks = None if row_block is None else blocks_of_rows(row_block)
    if blocks is not None and len(lengths) > 1 and not (np.diff(starts[:, 0]) >= 0).all():
        blocks = None                                    # (row ranges of another order: recomputed, as the reference does)
    if blocks is None and (len(lengths) == 0 or (starts == -1).any(axis=1).all()):
        print("No strict MUMs found after filtering. Aborting.", file=sys.stderr)
        return 0
    import mumemto_amd                         # (the library loads here: --help works without it)
    try:
        eng = mumemto_amd.Engine(args.device)
    except mumemto_amd.MumemtoError as ex:     # no usable GPU, or no library: there is no host fallback
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    try:
        with mumemto_amd.Merged.from_rows(eng, lengths, starts, strands) as m:
            if blocks is not None:
                print("Using pre-computed collinear blocks: %d blocks" % len(blocks), file=sys.stderr)
                m.set_blocks(blocks)
            else:
                if args.verbose:
                    print("Finding collinear blocks (max gap = %s bp)..." % (args.max_block_gap or None), file=sys.stderr)
                m.collinear(args.max_block_gap, None)
            if args.verbose:
                print("Finding inversions...", file=sys.stderr)
            calls = m.inversions(args.max_length)
    except mumemto_amd.MumemtoError as ex:
        print("Error: %s" % ex, file=sys.stderr)
        return 1
    finally:
        eng.close()
    if args.verbose:
        print("Found %d inversions" % len(calls), file=sys.stderr)
        print("Writing results...", file=sys.stderr)
    if len(calls) and int(calls[:, 0].max()) >= len(hap_ids):
        print("Error: %s names %d sequences, the table has %d" % (args.filelist, len(hap_ids), starts.shape[1]), file=sys.stderr)
        return 1
    try:
        sys.stdout.write(format_calls(calls, hap_ids, breaks, args.margin))
        sys.stdout.flush()
    except BrokenPipeError:
        os.dup2(os.open(os.devnull, os.O_WRONLY), sys.stdout.fileno())
    return 0


class _CallableModule(types.ModuleType):
    """`import mumemto_amd.find_inversions` binds this module over the function of the same name in the package: calls go on"""

    def __call__(self, *args, **kwargs):
        from .binding import find_inversions
        return find_inversions(*args, **kwargs)


if __name__ == "__main__":
    sys.exit(main(parse_arguments()))
else:
    sys.modules[__name__].__class__ = _CallableModule
