"""Host model of the inversion caller, in closed form (numpy), on top of collmodel.prepare / collmodel.blocks.

What the reference computes (mumemto/find_inversions.py main, find_reversals, inversion_coords on the block order of
mumemto/utils.py:62 / :67) over a prepared table and its blocks (l_b, r_b), for every column i >= 1:

  * order_i = the block numbers in ascending order of starts[l_b, i] (ties by b here: a stable sort; the reference leaves
    them to an unstable one, so no test table has any);
  * dec[j] = order_i[j + 1] - order_i[j] == -1; a run is a maximal stretch j = s .. e of true dec, positions s .. e + 1;
  * the run is kept when strands[l_b, i] is '-' for every block b of order_i[s .. e + 1];
  * first = order_i[s], last = order_i[e + 1]: (i, starts[r_first, i], starts[l_last, i] + length[l_last],
    starts[r_first, 0], starts[l_last, 0] + length[l_last]);
  * with max_length = L kept iff |end - start| <= L; calls in order of (i, s).
"""
import os

import numpy as np

import collmodel

HEADER = "hap_id\tstart\tend\tref_start\tref_end"


def runs(order):
    """[(s, e)] inclusive ranges of dec over one column's block order"""
    order = np.asarray(order, np.int64)
    if len(order) < 2:
        return []
    dec = np.concatenate(([False], np.diff(order) == -1, [False]))
    step = np.diff(dec.astype(np.int8))
    return list(zip(np.nonzero(step == 1)[0].tolist(), (np.nonzero(step == -1)[0] - 1).tolist()))


def calls(lengths, starts, strands, blk, max_length=None, counts=None):
    """int64 [k, 5] over a prepared table and its (n_blocks, 2) blocks; counts, a dict, receives runs / cols_sorted /
    cols_ascending as the device path counts them"""
    blk = np.asarray(blk, np.int64).reshape(-1, 2)
    lens = np.asarray(lengths, np.int64)
    starts = np.asarray(starts, np.int64)
    out = []
    n_runs = n_sorted = 0
    N = starts.shape[1] if starts.ndim == 2 else 0
    for i in range(1, N):
        if len(blk) < 2:
            break
        keys = starts[blk[:, 0], i]
        if (np.diff(keys) >= 0).all():
            continue                                    # the identity: no run
        n_sorted += 1
        order = np.argsort(keys, kind="stable")
        for s, e in runs(order):
            n_runs += 1
            if strands[blk[order[s:e + 2], 0], i].any():
                continue
            ra, rb = blk[order[s], 1], blk[order[e + 1], 0]
            rec = (i, starts[ra, i], starts[rb, i] + lens[rb], starts[ra, 0], starts[rb, 0] + lens[rb])
            if max_length is None or abs(int(rec[2]) - int(rec[1])) <= max_length:
                out.append(rec)
    if counts is not None:
        done = len(blk) >= 2 and N >= 2
        counts.update(runs=n_runs, cols_sorted=n_sorted, cols_ascending=max(N - 1, 0) - n_sorted if done else max(N - 1, 0))
    return np.array(out, np.int64).reshape(-1, 5)


def find(lengths, starts, strands, max_block_gap=1000, max_length=None):
    """a raw table -> calls, as the tool computes them: prepared, blocks without singletons, calls"""
    rows = collmodel.prepare(lengths, starts, strands)
    return calls(*rows, collmodel.blocks(*rows, max_break=max_block_gap), max_length=max_length)


def sequence_names(path, chrom=None):
    lines = [l.split() for l in open(path).read().splitlines()]
    if lines and len(lines[0]) > 1 and lines[0][1] == "*":
        lines = [l for l in lines if l[1] == "*"]
    names = [os.path.basename(l[0]) for l in lines]
    return [n.split("_chr%s" % chrom)[0] for n in names] if chrom else names


def scaffold_breaks(agp_filelist, chrom, hap_ids):
    """{hap_id: (running sums of end - start + 1 over the `W` lines of chr<C>, their component names)}"""
    out = {}
    for k, line in enumerate(open(agp_filelist).read().splitlines()):
        if k + 1 >= len(hap_ids) or not line.strip() or not os.path.exists(line.strip()):
            continue
        rows = [l.split() for l in open(line.strip()).read().splitlines() if l.startswith("chr%s" % chrom)]
        rows = [r for r in rows if r[4] == "W"]
        out[hap_ids[k + 1]] = (np.cumsum([int(r[2]) - int(r[1]) + 1 for r in rows]).tolist(), [r[5] for r in rows])
    return out


def stdout_bytes(call_rows, hap_ids, breaks=None, margin=0.01):
    """what the tool prints: the header, then one line per call"""
    lines = [HEADER + ("\tscaffold_break\tcontig" if breaks is not None else "")]
    for i, start, end, ref_start, ref_end in np.asarray(call_rows, np.int64).reshape(-1, 5).tolist():
        line = "\t".join([hap_ids[i]] + [str(v) for v in (start, end, ref_start, ref_end)])
        if breaks is not None and hap_ids[i] in breaks:
            at, names = breaks[hap_ids[i]]
            near = (end - start) * margin
            hit = [nm for p, nm in zip(at, names) if abs(p - start) < near] + [nm for p, nm in zip(at, names) if abs(p - end) < near]
            line += "\t%s\t%s" % ("True" if hit else "False", ",".join(hit) if hit else "NA")
        lines.append(line)
    return ("\n".join(lines) + "\n").encode()


# ---- tables whose blocks are given outright ------------------------------------------------------------------------
def block_table(columns, rows_per_block=2, bases=None):
    """A prepared table and its blocks: block b holds rows_per_block rows, column 0 ascends, and in column c + 1 the blocks lie
    in the order columns[c][0] (order[j] = block at position j) on the strands columns[c][1] (per block, True = '+'); rows of a
    '-' block descend.  bases[c] is added to every start of column c (column 0 included)."""
    B = len(columns[0][0])
    n, N = B * rows_per_block, len(columns) + 1
    lens = (10 + np.arange(n) % 7).astype(np.uint32)
    starts = np.zeros((n, N), np.int64)
    strands = np.ones((n, N), bool)
    starts[:, 0] = np.arange(n) * 100
    within = np.tile(np.arange(rows_per_block), B)
    for c, (order, plus_of_block) in enumerate(columns, start=1):
        pos = np.empty(B, np.int64)
        pos[np.asarray(order, np.int64)] = np.arange(B)
        plus = np.repeat(np.asarray(plus_of_block, bool), rows_per_block)
        starts[:, c] = np.repeat(pos, rows_per_block) * 1000 + np.where(plus, within, rows_per_block - 1 - within) * 100 + 7
        strands[:, c] = plus
    if bases is not None:
        starts += np.asarray(bases, np.int64)[None, :]
    first = np.arange(B) * rows_per_block
    return (lens, starts, strands), np.stack([first, first + rows_per_block - 1], axis=1).astype(np.uint32).reshape(-1, 2)


def reversed_segments(B, segments):
    """the identity order of B blocks with every inclusive (first, last) range of positions reversed in place"""
    order = np.arange(B)
    for a, b in segments:
        order[a:b + 1] = order[a:b + 1][::-1].copy()
    return order


# ---- the recorded runs of tests/golden/inversion ----------------------------------------------------------------------
def fixture_runs(gold):
    """runs.json: [{out, flags, calls, agp}] -- flags as the reference's tool got them, file names relative to the directory,
    AGPLIST standing for a list of the paths under `agp`"""
    import json
    return json.load(open(os.path.join(gold, "runs.json")))


def real_flags(run, gold, tmp_dir):
    """the flags of a recorded run with real paths; the AGP list is written into tmp_dir"""
    out = []
    for f in run["flags"]:
        if f == "AGPLIST":
            path = os.path.join(str(tmp_dir), "agp_list.txt")
            open(path, "w").write("".join(os.path.join(gold, p) + "\n" for p in run["agp"]))
            out.append(path)
        elif os.path.exists(os.path.join(gold, f)) or os.path.exists(os.path.join(gold, f + ".mums")):
            out.append(os.path.join(gold, f))
        else:
            out.append(f)
    return out


def table_and_blocks(path):
    """a .mums / .bumbl file -> (raw table, blocks the file carries or None), as the tool reads it: blocks over rows that are
    not in order of column 0 are dropped"""
    from mumemto_amd import mumsio
    if path.endswith(".bumbl"):
        lengths, starts, strands, blk = mumsio.read_bumbl(path, with_blocks=True)
    else:
        lengths, starts, strands, rb = mumsio.read_mums(path, with_blocks=True)
        blk = None
        if rb is not None:
            rb = rb.astype(np.int64)
            cut = np.nonzero(np.diff(rb) != 0)[0] + 1
            first, last = np.concatenate(([0], cut)), np.concatenate((cut - 1, [len(rb) - 1]))
            keep = rb[first] != mumsio.NO_BLOCK
            blk = np.stack([first[keep], last[keep]], axis=1).astype(np.uint32)
    if blk is not None and len(lengths) > 1 and not (np.diff(starts[:, 0]) >= 0).all():
        blk = None
    return (lengths, starts, strands), blk


def run_calls(args):
    """the calls of a run from the model: args as mumemto_amd.find_inversions.parse_arguments returns them"""
    table, blk = table_and_blocks(args.mumfile)
    if blk is not None:
        return calls(*table, blk, max_length=args.max_length)
    return find(*table, max_block_gap=args.max_block_gap, max_length=args.max_length)


def run_stdout(args):
    hap_ids = sequence_names(args.filelist, args.chr)
    breaks = scaffold_breaks(args.agp_filelist, args.chr, hap_ids) if args.agp_filelist else None
    return stdout_bytes(run_calls(args), hap_ids, breaks, args.margin)
