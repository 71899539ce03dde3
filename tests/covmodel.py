"""The coverage of a sequence by multi-MUMs in closed form (numpy), the model of csrc/coverage.cpp; a naive bitmap, the
reference's own method (mumemto/mum_coverage.py); a seeded generator of tables with the shapes chain tables lack; and the
helpers of the recorded fixtures (tests/golden/coverage).

Column c, sequence length L, length filter F: a row takes part when start != -1 and length >= F, its interval is
[start, min(start + length, L)).  In ascending order of the start, prev = the maximum of all earlier ends (minus infinity for
the first): an interval adds max(0, end - max(start, prev)), and begins a run when start > prev."""
import json
import os

import numpy as np


def intervals(lengths, col_starts, L, F=0):
    """the non-empty intervals of one column, in ascending order of the start: (begin, end) int64 arrays"""
    s = np.asarray(col_starts, np.int64)
    ln = np.asarray(lengths, np.int64)
    keep = (s != -1) & (ln >= F)
    b = s[keep]
    e = np.minimum(b + ln[keep], L)
    ok = e > b
    b, e = b[ok], e[ok]
    order = np.argsort(b, kind="stable")
    return b[order], e[order]


def column(lengths, col_starts, L, F=0):
    """-> (covered, runs int64 [k, 2]) of one column"""
    b, e = intervals(lengths, col_starts, L, F)
    if not len(b):
        return 0, np.zeros((0, 2), np.int64)
    top = np.maximum.accumulate(e)
    prev = np.concatenate(([-1], top[:-1]))
    covered = int(np.maximum(0, e - np.maximum(b, prev)).sum())
    head = np.nonzero(b > prev)[0]
    ends = np.concatenate((top[head[1:] - 1], top[-1:]))
    return covered, np.stack([b[head], ends], axis=1)


def coverage(lengths, starts, seq_lengths, seq_idx=None, min_length=0):
    """what Merged.coverage + Merged.coverage_runs return: (covered u64 [N], run_begin u64 [N + 1], runs i64 [n, 2])"""
    starts = np.asarray(starts, np.int64)
    nd = starts.shape[1]
    covered, run_begin, runs = np.zeros(nd, np.uint64), np.zeros(nd + 1, np.uint64), [np.zeros((0, 2), np.int64)]
    for c in range(nd):
        if seq_idx is None or c == seq_idx:
            covered[c], r = column(lengths, starts[:, c], int(seq_lengths[c]), min_length)
            runs.append(r)
        run_begin[c + 1] = sum(len(r) for r in runs)
    return covered, run_begin, np.concatenate(runs)


def bitmap(lengths, col_starts, L, F=0):
    """the reference's method: one bool per base, a slice set per row"""
    cov = np.zeros(L, bool)
    for ln, s in zip(np.asarray(lengths).tolist(), np.asarray(col_starts).tolist()):
        if s != -1 and ln >= F:
            cov[s:s + ln] = True
    return cov


def runs_of_bitmap(cov):
    d = np.diff(np.concatenate(([0], cov.astype(np.int8), [0])))
    return np.stack([np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]], axis=1).astype(np.int64).reshape(-1, 2)


def make_table(seed, n, n_docs, max_len=400, density=0.6, absent=0.1, base=0, absent_columns=()):
    """-> (lengths u32 [n], starts i64 [n, N], strands bool [n, N], seq_lengths i64 [N]).  Random intervals at a density that
    leaves the coverage strictly between 0 and 100 %: they overlap; a twentieth of the rows is eight times as long (others
    nest in them); a tenth repeats the row before (duplicates); a tenth starts where the row before ends (touching); `absent`
    of the cells are -1; a few rows run over the end of the sequence, a few start at it or beyond; the columns of
    absent_columns are -1 throughout.  base is added to every start and sequence length (starts beyond 2^32)."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, max_len, n).astype(np.uint32)
    lengths[rng.random(n) < 0.05] *= 8
    seq_lengths = np.maximum(1, (rng.integers(90, 110, n_docs) * int(lengths.sum() / density)) // 100).astype(np.int64)
    starts = np.stack([rng.integers(0, L, n) for L in seq_lengths], axis=1).astype(np.int64).reshape(n, n_docs)
    for r in np.nonzero(rng.random(n) < 0.1)[0]:
        if r:
            starts[r] = starts[r - 1]
            lengths[r] = lengths[r - 1]
    for r in np.nonzero(rng.random(n) < 0.1)[0]:
        if r:
            starts[r] = starts[r - 1] + int(lengths[r - 1])
    for r in np.nonzero(rng.random(n) < 0.03)[0]:
        c = int(rng.integers(0, n_docs))
        starts[r, c] = seq_lengths[c] - int(rng.integers(0, lengths[r] + 1))          # over the end, or exactly up to it
    for r in np.nonzero(rng.random(n) < 0.03)[0]:
        c = int(rng.integers(0, n_docs))
        starts[r, c] = seq_lengths[c] + int(rng.integers(0, 3))                       # at the end, or beyond
    starts[rng.random((n, n_docs)) < absent] = -1
    starts[:, list(absent_columns)] = -1
    starts[starts != -1] += base
    return lengths, starts, rng.random((n, n_docs)) < 0.5, seq_lengths + base


# ---- the recorded fixtures ---------------------------------------------------------------------------------------------
def fixture_runs(gold):
    return json.load(open(os.path.join(gold, "runs.json")))


def real_flags(run, gold):
    """the flags of a run with the file names made absolute"""
    return [os.path.join(gold, f[5:]) if f.startswith("GOLD/") else f for f in run["flags"]]


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


def stderr_line(idx, covered, L):
    return ("seq%d: %.3f%%\n" % (idx, int(covered) * 100 / int(L))).encode()
