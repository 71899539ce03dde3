"""Built anchor partitions for the fold (the partition merge) and the fold itself in plain Python integers.

partitions(seed) writes row tables and threshold columns directly -- no sequences behind them -- so that the fold meets
what natural partitions hardly ever hold: a merged length equal to the merged threshold, merged lengths 19 / 20 / 21, a
short row that started inside a long one, rows at anchor position 0 and at the last one, anchor lengths at a power of
two, a threshold of 0 on one side only, a partition without rows, offsets beyond 2^32, 130 output columns.

fold(parts, min_len) follows merge_partitions of the reference (src/merge_candidates.cpp:97-157) as a specification;
tests/test_fold_host.py holds it to the reference's own anchor_merge binary on every case.

Anchor starts are distinct within a partition: the reference takes the next row of its sorted table for every set bit
of its start vector (merge_candidates.cpp:126-133), so two rows on one start leave it one row behind for the rest of
the anchor -- the reference is out of step with itself there, and such tables are out of scope.
"""
import os

import numpy as np

from mumsfile import format_mums

LENS = (1, 19, 20, 21, 22, 25, 40, 80, 300)
LEN_W = (1, 2, 3, 3, 2, 3, 4, 3, 2)
THR = (0, 1, 5, 18, 19, 20, 21, 24, 39, 40, 79, 65535)
THR_P = (.03, .30, .20, .15, .08, .06, .04, .04, .03, .03, .02, .02)     # skewed low: rows have to survive 1 - 5 steps
ANCHORS = (40, 256, 257, 4096, 4097, 70001)
WINDOW, FENCE = 64, 300
OFF_END = 1 << 41

# ---- the fold ---------------------------------------------------------------------------------------------------------


def _side(p):
    rows = sorted((int(o[0]), int(l), [int(x) for x in o], [int(x) for x in s]) for l, o, s in zip(p[0], p[1], p[2]))
    return rows, [int(t) for t in p[3]]


def _fold_step(r1, t1, r2, t2, min_len):
    """rows: (start, length, offsets, strands) in anchor order; merge_candidates.cpp:106-157 line by line"""
    at1, at2 = {r[0]: r for r in r1}, {r[0]: r for r in r2}
    cur1 = cur2 = None
    rows, t = [], [0] * len(t1)
    for i in range(len(t1)):
        both = t1[i] > 0 and t2[i] > 0
        if both:
            t[i] = max(t1[i], t2[i])
        cur1, cur2 = at1.get(i, cur1), at2.get(i, cur2)      # the last row that started at or before i
        if cur1 is None or cur2 is None or not (i in at1 or i in at2) or not both:
            continue
        d1, d2 = i - cur1[0], i - cur2[0]
        if d1 > cur1[1] or d2 > cur2[1]:
            continue
        s1, s2 = cur1[1] - d1, cur2[1] - d2
        n = min(s1, s2)
        if n > t[i] and n >= min_len:
            o1 = [o + (d1 if s else s1 - n) for o, s in zip(cur1[2], cur1[3])]     # fix_neg_strand, :97-104
            o2 = [o + (d2 if s else s2 - n) for o, s in zip(cur2[2], cur2[3])]
            rows.append((i, n, o1 + o2[1:], cur1[3] + cur2[3][1:]))
    return rows, t


def fold(parts, min_len=20):
    """parts: [(length, offsets[n, nd], strands[n, nd], thresh)] -> (length u32[m], offsets i64[m, N], strands u8[m, N],
    thresh i64[L]) of the merged table, rows in anchor order, thresholds at whatever size they come out."""
    rows, t = _side(parts[0])
    n_docs = parts[0][1].shape[1]
    for p in parts[1:]:
        r2, t2 = _side(p)
        rows, t = _fold_step(rows, t, r2, t2, min_len)
        n_docs += p[1].shape[1] - 1
    return (np.array([r[1] for r in rows], np.uint32), np.array([r[2] for r in rows], np.int64).reshape(len(rows), n_docs),
            np.array([r[3] for r in rows], np.uint8).reshape(len(rows), n_docs), np.array(t, np.int64))


def saturated(parts):
    """the same partitions with their thresholds as PREFIX.athresh holds them: 16 bits, 65535 for anything above"""
    return [(p[0], p[1], p[2], np.minimum(p[3], 65535).astype(np.uint16)) for p in parts]


def write_set(directory, parts):
    """p00.mums / p00.athresh, p01... (the inputs of the anchor_merge tools) -> the .mums paths in order"""
    paths = []
    for g, (length, off, st, th) in enumerate(parts):
        base = os.path.join(str(directory), "p%02d" % g)
        with open(base + ".mums", "wb") as f:
            f.write(format_mums(length, off, st))
        np.asarray(th).astype(np.uint16).tofile(base + ".athresh")
        paths.append(base + ".mums")
    return paths


# ---- the generator ----------------------------------------------------------------------------------------------------
# Constructs: each lives in a window of 64 anchor positions at the front of the anchor, carried by two partitions a < b
# (rows and threshold overrides below, positions relative to the window).  Every other partition has one row of 300 on
# the window's first position and thresholds of 1, so that it neither trims nor vetoes; a and b start a row there too,
# which ends whatever reaches in from the window before.  `want` is what the whole fold must hold at min_len 20: the
# merged length of the row that starts at that position, 0 for no row.
CONSTRUCTS = {
    # merged length == merged threshold: no row; one above: a row.  Position 1 starts one behind b's row.
    "equal": dict(a=[(0, 40), (1, 40), (9, 40), (12, 40), (15, 40), (18, 40)],
                  b=[(0, 25), (5, 25), (9, 21), (12, 21), (15, 20), (18, 20)],
                  ta={1: 24, 5: 24, 15: 20, 18: 19}, tb={1: 5, 9: 21, 12: 20},
                  want={0: 25, 1: 0, 5: 25, 9: 0, 12: 21, 15: 0, 18: 20}),
    "len192021": dict(a=[(0, 80)], b=[(0, 80), (4, 19), (8, 20), (12, 21), (16, 22)], ta={}, tb={16: 21},
                      want={0: 80, 4: 0, 8: 20, 12: 21, 16: 22}),
    # the last row that started at or before i decides, not the longest one that covers i
    "nested": dict(a=[(0, 80), (2, 20), (30, 80), (32, 22)], b=[(0, 80), (24, 25), (35, 25)], ta={}, tb={},
                   want={2: 20, 24: 0, 30: 0, 32: 0, 35: 0}),
    # a's rows start 1, len and len + 1 behind b's row of 22
    "delta": dict(a=[(0, 80), (1, 40), (22, 25), (23, 25)], b=[(0, 22)], ta={}, tb={},
                  want={0: 22, 1: 21, 22: 0, 23: 0}),
    "zero_one_side": dict(a=[(0, 80), (6, 25), (9, 25), (12, 25)], b=[(0, 80), (6, 25), (9, 25), (12, 25)],
                          ta={6: 0, 9: 5}, tb={6: 5, 9: 5, 12: 0}, want={6: 0, 9: 25, 12: 0}),
}
NAMES = tuple(CONSTRUCTS)


def _offsets(rng, n, nd):
    """anchor column left empty; the others anywhere in [0, 2^41), half of them with 1 - 13 digits at equal odds"""
    off = rng.integers(0, OFF_END, size=(n, nd), dtype=np.int64)
    digits = rng.integers(1, 14, size=(n, nd))
    short = np.minimum((rng.random((n, nd)) * 10.0 ** digits).astype(np.int64), OFF_END - 1)
    return np.where(rng.random((n, nd)) < 0.5, short, off)


def _table(rng, rows, nd):
    """{start: length} -> (length, offsets, strands) in shuffled order (a .mums file is in match-string order)"""
    starts = np.array(sorted(rows), np.int64)
    starts = starts[rng.permutation(len(starts))]
    off = _offsets(rng, len(starts), nd)
    st = rng.integers(0, 2, size=(len(starts), nd)).astype(np.uint8)
    off[:, 0], st[:, 0] = starts, 1
    return np.array([rows[int(s)] for s in starts], np.uint32), off, st


def _random_region(rng, rows, thr, lo, hi, low):
    """rows {start: length} and thresholds of every partition over [lo, hi): starts mostly from a pool the partitions
    share (a fold makes a row only where both sides have one running), gaps of 1 - 60, a few far out and a few private"""
    k = len(rows)
    if hi <= lo:
        return
    pool, x = [], lo
    while x < hi and len(pool) < 240:
        pool.append(x)
        x += int(rng.choice((1, 2, 3, 5, 8, 13, 21, 34, 60)))
    if hi - lo > 5000:
        pool += [int(v) for v in rng.integers(lo, hi, 24)]
    pool = sorted(set(pool))
    lens = np.array(LENS)
    lw = np.array((0, 0, 1, 1, 1, 3, 4, 3, 2) if low else LEN_W, float)
    tp = np.array((0, .85, .1, .05, 0, 0, 0, 0, 0, 0, 0, 0) if low else THR_P, float)
    for g in range(k):
        thr[g][lo:hi] = rng.choice(THR, size=hi - lo, p=tp / tp.sum())
        mine = [p for p in pool if rng.random() < (0.9 if low else 0.8)]
        mine += [int(v) for v in rng.integers(lo, hi, int(rng.integers(3, 10)))]
        for s in mine:
            rows[g][s] = int(rng.choice(lens, p=lw / lw.sum()))
    if not low:
        for s in rng.choice(pool, size=min(4, len(pool)), replace=False):      # 0 on exactly one side at a row start
            z = int(rng.integers(0, k))
            for g in range(k):
                thr[g][s] = 0 if g == z else int(rng.choice((1, 5, 18)))
                rows[g].setdefault(int(s), 25)


def _shape(seed, rng):
    kind = "wide" if seed % 40 == 39 else "empty_mid" if seed % 10 == 3 else "empty_last" if seed % 10 == 8 else "plain"
    if kind == "wide":                          # 1 + 43 x 3 = 130 output columns
        return kind, 257, [3] * 43
    k = int(rng.integers(3 if kind == "empty_mid" else 2, 7))
    return kind, ANCHORS[seed % len(ANCHORS)], [int(rng.integers(1, 5)) for _ in range(k)]


def partitions(seed, further=None, anchor_len=None):
    """-> (parts, anchor length, constructs): parts = [(length u32[n], offsets i64[n, nd], strands u8[n, nd], thresh
    u16[anchor length])], column 0 the anchor ('+' always); constructs = {name: {anchor position: merged length the
    whole fold must hold there at min_len 20, 0 for no row}} of what was placed.  further / anchor_len: the numbers of
    non-anchor documents per partition and the anchor length, instead of what the seed picks."""
    rng = np.random.default_rng(seed)
    kind, L, docs = _shape(seed, rng)
    if further is not None:
        kind, docs = "plain", list(further)
    if anchor_len is not None:
        L = anchor_len
    k = len(docs)
    low = k > 6
    rows = [dict() for _ in range(k)]
    thr = [np.ones(L, np.int64) for _ in range(k)]
    constructs = {}
    names = [] if L < 256 or kind.startswith("empty") else \
        [NAMES[(seed // len(ANCHORS) + j) % len(NAMES)] for j in range(2)] if L < 1024 else [NAMES[j] for j in rng.permutation(len(NAMES))]
    for w, name in zip(range(0, WINDOW * len(names), WINDOW), names if k > 1 else []):
        c = CONSTRUCTS[name]
        a, b = sorted(int(x) for x in rng.choice(k, size=2, replace=False))
        for g in range(k):
            for s, n in (c["a"] if g == a else c["b"] if g == b else [(0, FENCE)]):
                rows[g][w + s] = n
        for s, t in c["ta"].items():
            thr[a][w + s] = t
        for s, t in c["tb"].items():
            thr[b][w + s] = t
        constructs[name] = {w + s: n for s, n in c["want"].items()}
    zone = WINDOW * len(constructs)
    _random_region(rng, rows, thr, zone, L - 1, low)
    for name, pos in (("first", 0), ("last", L - 1)):      # a row on the first position, and one on the last (past the end)
        if name == "first" and zone:
            continue
        n = [int(rng.choice((20, 21, 22, 25, 40))) for _ in range(k)]
        for g in range(k):
            rows[g][pos], thr[g][pos] = n[g], 1
        constructs[name] = {pos: min(n)}
    if kind.startswith("empty"):
        rows[k // 2 if kind == "empty_mid" else k - 1] = {}
        constructs = {kind: {}}
    parts = [_table(rng, rows[g], docs[g] + 1) + (thr[g].astype(np.uint16),) for g in range(k)]
    return parts, L, constructs


# ---- the 32-bit flavour -----------------------------------------------------------------------------------------------
DECIDERS = ((70000, 70000), (70001, 70000), (70000, 70001), (65536, 65536), (65536, 65535), (69999, 69999), (70000, 69999))


def partitions32(seed):
    """Thresholds as the engine carries them (uint32, never saturated) -> (parts, anchor length, constructs).  On the
    first positions every partition starts a row of about 70,000; the shortest is the merged length, and one partition
    holds a threshold of 65,535 / 65,536 / 69,999 / 70,000 / 70,001 there, the others small ones.  Where the merged
    length is above 65,535 and not above the threshold, the fold makes no row -- and would make one from the same
    column saturated at 16 bits.  constructs = {"decider32": {position: 1 where the two differ, else 0}}."""
    rng = np.random.default_rng(1000 + seed)
    L = 70001 + seed % 3
    k = int(rng.integers(3, 6))
    docs = [int(rng.integers(1, 4)) for _ in range(k)]
    rows = [dict() for _ in range(k)]
    thr = [np.ones(L, np.int64) for _ in range(k)]
    differ = {}
    pos = 0
    for j in range(40):
        n, t = DECIDERS[j] if j < len(DECIDERS) else (int(rng.choice((65536, 69999, 70000, 70001, 70002))),
                                                       int(rng.choice((65535, 65536, 69999, 70000, 70001))))
        holder, shortest = int(rng.integers(0, k)), int(rng.integers(0, k))
        for g in range(k):
            rows[g][pos] = n if g == shortest else n + int(rng.integers(0, 12))
            thr[g][pos] = t if g == holder else int(rng.choice((1, 5, 79)))
        differ[pos] = int(n > 65535 and n <= t)
        pos += int(rng.integers(1, 12))
    _random_region(rng, rows, thr, 512, L - 1, False)
    for g in range(k):
        big = rng.integers(512, L - 1, 40)                  # thresholds above 16 bits under ordinary rows too
        thr[g][big] = rng.choice((65535, 65536, 70000), size=40)
    parts = [_table(rng, rows[g], docs[g] + 1) + (thr[g].astype(np.uint32),) for g in range(k)]
    return parts, L, {"decider32": differ}
