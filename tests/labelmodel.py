"""Host model of the contig labels (`mumemto label`, mumemto/get_sequence_info.py): a closed form (numpy) and a plain loop.

For the contigs (name_k, len_k) of column c, ends_k = len_0 + ... + len_k, cell (r, c) with start s gets

  * contig = the first k with ends_k > s (searchsorted, side='right'; a contig of length 0 is never chosen),
  * rel = s - (ends_k - len_k); s == -1: contig 0 (what searchsorted gives) and rel -1 (the reference's mask);
  * s >= ends[-1]: refused (OutOfRange names the first such cell in row-major order); the reference raises IndexError.

The line of a row: LEN \\t s_0,... \\t +|-,... \\t BLOCK \\t c_0,... \\t rel_0,... \\n with -1 printed for an absent start,
BLOCK = `*` without blocks, else the row's block or `-`, and c_j the decimal contig or, with names, names[j][contig].
"""
import numpy as np

from bedmodel import make_contigs, make_rows, row_blocks  # noqa: F401  (seeded inputs for the tests)
from collmodel import make_table  # noqa: F401

NO_BLOCK = 0xFFFFFFFF


class OutOfRange(Exception):
    def __init__(self, row, col, start, total):
        Exception.__init__(self, "the start %d of row %d, column %d lies at or beyond the total length %d of sequence %d"
                           % (start, row, col, total, col))
        self.row, self.col, self.start, self.total = row, col, start, total


def cells(starts, contig_lens):
    """-> (contig uint32 [n, N], rel int64 [n, N]); contig_lens: one list of contig lengths per column"""
    starts = np.asarray(starts, np.int64)
    n, n_docs = starts.shape
    contig = np.zeros((n, n_docs), np.uint32)
    rel = np.zeros((n, n_docs), np.int64)
    beyond = np.zeros((n, n_docs), bool)
    for c in range(n_docs):
        lens = np.asarray(contig_lens[c], np.int64)
        ends = np.cumsum(lens)
        k = np.searchsorted(ends, starts[:, c], side="right")
        beyond[:, c] = k >= len(ends)
        k = np.minimum(k, len(ends) - 1)
        contig[:, c] = k
        rel[:, c] = starts[:, c] - np.hstack((0, ends[:-1]))[k]
    if beyond.any():
        r, c = np.argwhere(beyond)[0].tolist()               # (argwhere lists in row-major order)
        raise OutOfRange(r, c, int(starts[r, c]), int(np.sum(contig_lens[c])))
    rel[starts == -1] = -1
    return contig, rel


def text(lengths, starts, strands, contig, rel, blocks=None, names=None):
    """the bytes of the labelled table; blocks: None, or the (n_blocks, 2) list attached; names: None, or one list per column"""
    n = len(lengths)
    strands = np.asarray(strands).astype(bool).reshape(contig.shape)
    rb = None if blocks is None else row_blocks(blocks, n).tolist()
    out = []
    for r, (length, row, srow, crow, rrow) in enumerate(zip(np.asarray(lengths).tolist(), np.asarray(starts).tolist(),
                                                            strands.tolist(), contig.tolist(), rel.tolist())):
        block = "*" if rb is None else "-" if rb[r] == NO_BLOCK else str(rb[r])
        field5 = [str(k) for k in crow] if names is None else [names[c][k] for c, k in enumerate(crow)]
        out.append("%d\t%s\t%s\t%s\t%s\t%s\n" % (length, ",".join(map(str, row)), ",".join("+" if s else "-" for s in srow), block,
                                                 ",".join(field5), ",".join(map(str, rrow))))
    return "".join(out).encode()


def label(lengths, starts, strands, contigs, blocks=None, names=False):
    """what Merged.label leaves: (contig, rel, text)"""
    starts = np.asarray(starts, np.int64).reshape(len(lengths), len(contigs[1]))
    contig, rel = cells(starts, contigs[1])
    return contig, rel, text(lengths, starts, strands, contig, rel, blocks, contigs[0] if names else None)


def loop_label(lengths, starts, strands, contigs, blocks=None, names=False):
    """the same one cell at a time, without numpy's search"""
    block_of = {}
    for b, (lo, hi) in enumerate([] if blocks is None else np.asarray(blocks).tolist()):
        for r in range(lo, hi + 1):
            block_of[r] = b
    lines = []
    for r in range(len(lengths)):
        f2, f3, f5, f6 = [], [], [], []
        for c in range(len(contigs[1])):
            s = int(starts[r][c])
            total, k, left = 0, None, 0
            for j, v in enumerate(contigs[1][c]):
                total += v
                if total > s:
                    k, left = j, total - v
                    break
            if k is None:
                raise OutOfRange(r, c, s, total)
            f2.append(str(s))
            f3.append("+" if strands[r][c] else "-")
            f5.append(contigs[0][c][k] if names else str(k))
            f6.append(str(-1 if s == -1 else s - left))
        block = "*" if blocks is None else str(block_of.get(r, "-"))
        lines.append("\t".join([str(int(lengths[r])), ",".join(f2), ",".join(f3), block, ",".join(f5), ",".join(f6)]) + "\n")
    return "".join(lines).encode()
