"""The MEM density of the sequences in closed form (numpy difference arrays), the model of csrc/density.cpp; a plain triple
loop over a num x size array, the reference's own method (mumemto/mem_density.py) without numpy's slices; a seeded generator
of MEM rows; and the helpers of the recorded fixtures (tests/golden/density).

size = max(seq_lengths).  An occurrence (doc, start) of a row of length l covers, in doc, what the numpy slice
start : start + l selects on an axis of `size` entries: a = start + size clamped below at 0 for a negative start, else start
clamped above at size; b by the same rule from start + l; [a, b) when a < b.  Bin k is [k W, min((k + 1) W, size))."""
import os

import numpy as np


def slice_bounds(starts, ls, size):
    """(a, b) int64 arrays: the slice rule, element by element"""
    starts = np.asarray(starts, np.int64)
    stops = starts + np.asarray(ls, np.int64)

    def clamp(v):
        return np.where(v < 0, np.maximum(v + size, 0), np.minimum(v, size))
    return clamp(starts), clamp(stops)


def per_occurrence(lengths, occ_start):
    """the length of its row for every occurrence of the flat list"""
    occ_start = np.asarray(occ_start, np.int64)
    return np.repeat(np.asarray(lengths, np.int64), np.diff(occ_start))


def per_base(lengths, occ_start, starts, docs, seq_lengths):
    """int64 [num, size]: the depth of every position, by one difference array per sequence"""
    num, size = len(seq_lengths), int(max(seq_lengths))
    a, b = slice_bounds(starts, per_occurrence(lengths, occ_start), size)
    keep = a < b
    docs = np.asarray(docs, np.int64)[keep]
    diff = np.zeros((num, size + 1), np.int64)
    np.add.at(diff, (docs, a[keep]), 1)
    np.add.at(diff, (docs, b[keep]), -1)
    return np.cumsum(diff, axis=1)[:, :size]


def nbins_of(size, W):
    W = min(int(W), size)
    return (size + W - 1) // W


def binned(lengths, occ_start, starts, docs, seq_lengths, W):
    """uint64 [num, nbins]: the depth summed over every bin, without the per-base array.  An interval [a, b) gives bin k
    max(0, min(b, hi_k) - max(a, lo_k)) positions: with F(x)[k] = clip(x - lo_k, 0, hi_k - lo_k), the positions of the bin
    below x, that is F(b)[k] - F(a)[k], and F(x) is one whole bin width for every bin before bin(x) plus x - lo in bin(x)."""
    num, size = len(seq_lengths), int(max(seq_lengths))
    W = min(int(W), size)
    nb = (size + W - 1) // W
    a, b = slice_bounds(starts, per_occurrence(lengths, occ_start), size)
    keep = a < b
    a, b, docs = a[keep], b[keep], np.asarray(docs, np.int64)[keep]
    lo = np.arange(nb, dtype=np.int64) * W
    width = np.minimum(lo + W, size) - lo
    count = np.zeros((num, nb + 1), np.int64)        # count[q, k]: the ends x in bin k, +1 for a b and -1 for an a
    part = np.zeros((num, nb + 1), np.int64)         # part[q, k]: the sum of +-(x - lo_k) over those ends
    for x, sign in ((b, 1), (a, -1)):
        k = x // W                                   # (x = size where W divides it: bin nb, the spare column)
        np.add.at(count, (docs, k), sign)
        np.add.at(part, (docs, k), sign * (x - k * W))
    # every end in a bin beyond k gives bin k its whole width: the sum of `count` strictly behind k
    beyond = np.cumsum(count[:, ::-1], axis=1)[:, ::-1]
    out = beyond[:, 1:] * width + part[:, :nb]
    assert (out >= 0).all()
    return out.astype(np.uint64)


def sum_by_bins(base, W):
    """the per-base array summed over bins of W positions: uint64 [num, nbins]"""
    num, size = base.shape
    W = min(int(W), size)
    nb = (size + W - 1) // W
    padded = np.zeros((num, nb * W), np.int64)
    padded[:, :size] = base
    return padded.reshape(num, nb, W).sum(axis=2).astype(np.uint64)


def loop(lengths, occ_start, starts, docs, seq_lengths):
    """float64 [num, size] by three plain loops: rows, occurrences, positions"""
    num, size = len(seq_lengths), int(max(seq_lengths))
    cov = np.zeros((num, size))
    for r in range(len(lengths)):
        ln = int(lengths[r])
        for i in range(int(occ_start[r]), int(occ_start[r + 1])):
            start, stop = int(starts[i]), int(starts[i]) + ln
            a = max(start + size, 0) if start < 0 else min(start, size)
            b = max(stop + size, 0) if stop < 0 else min(stop, size)
            for x in range(a, b):
                cov[int(docs[i]), x] += 1
    return cov


def stats(lengths, occ_start, starts, docs, seq_lengths):
    """what Density.stats counts: occurrences, cut (start + l beyond size), empty (covered nothing), negative starts"""
    size = int(max(seq_lengths))
    ls = per_occurrence(lengths, occ_start)
    starts = np.asarray(starts, np.int64)
    a, b = slice_bounds(starts, ls, size)
    return dict(occurrences=len(starts), cut=int((starts + ls > size).sum()), empty=int((a >= b).sum()),
                negative=int((starts < 0).sum()))


def make_rows(seed, n_rows, num, size, max_len=None, occ=(2, 9), edge=0.15):
    """-> (lengths u32 [n], occ_start u64 [n + 1], starts i64 [T], docs u64 [T]): seeded MEM rows over `num` sequences of up
    to `size` positions; a share `edge` of the occurrences starts below 0, at size, beyond it, or ends exactly at size"""
    rng = np.random.default_rng(seed)
    max_len = max_len or max(2, size // 3)
    lengths = rng.integers(1, max_len + 1, n_rows).astype(np.uint32)
    counts = rng.integers(occ[0], occ[1] + 1, n_rows)
    occ_start = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    total = int(occ_start[-1])
    ls = np.repeat(lengths.astype(np.int64), counts)
    starts = rng.integers(0, size, total).astype(np.int64)
    kind = rng.random(total)
    starts = np.where(kind < edge * 0.25, -rng.integers(1, 2 * size + 2, total), starts)
    starts = np.where((kind >= edge * 0.25) & (kind < edge * 0.5), size + rng.integers(0, 3, total), starts)
    starts = np.where((kind >= edge * 0.5) & (kind < edge), size - ls, starts)            # ends exactly at size (or wraps)
    docs = rng.integers(0, num, total).astype(np.uint64)
    return lengths, occ_start, starts.astype(np.int64), docs


def mems_bytes(lengths, occ_start, starts, docs, strands=None):
    """the lines of a PREFIX.mems file: length <TAB> starts <TAB> documents <TAB> strands"""
    out = []
    for r in range(len(lengths)):
        i, j = int(occ_start[r]), int(occ_start[r + 1])
        st = ["+"] * (j - i) if strands is None else ["+" if s else "-" for s in strands[i:j]]
        out.append("%d\t%s\t%s\t%s\n" % (int(lengths[r]), ",".join(str(int(v)) for v in starts[i:j]),
                                        ",".join(str(int(v)) for v in docs[i:j]), ",".join(st)))
    return "".join(out).encode()


# ---- the recorded fixtures ---------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density")
FIXTURES = ("wraps", "edges", "short_seq", "multifasta")


def fixture_paths(name):
    return tuple(os.path.join(GOLD, name + ext) for ext in (".mems", ".lengths", "_coverage.npy"))


def sequence_lengths(path):
    """the second field of every line; of a multi-FASTA lengths file the sum of the third fields of a sequence's contig lines"""
    lines = [l.split() for l in open(path).read().splitlines()]
    if lines[0][1] != "*":
        return [int(l[1]) for l in lines]
    out = []
    for l in lines:
        if l[1] == "*":
            out.append(0)
        else:
            out[-1] += int(l[2])
    return out


def read_mems_plain(path):
    """a .mems file by per-line Python (the yardstick of mumsio.read_mems): the four arrays of make_rows"""
    lengths, occ_start, starts, docs = [], [0], [], []
    for line in open(path):
        f = line.split()
        if not f:
            continue
        lengths.append(int(f[0]))
        starts += [int(v) for v in f[1].split(",")]
        docs += [int(v) for v in f[2].split(",")]
        occ_start.append(len(starts))
    return np.array(lengths, np.uint32), np.array(occ_start, np.uint64), np.array(starts, np.int64), np.array(docs, np.uint64)
