"""Host model of the collinear blocks of multi-MUMs, in closed form (numpy), and seeded tables for its tests.

What the reference computes (mumemto/utils.py:9-64 find_coll_blocks on a table prepared by MUMdata.sort and
MUMdata.filter_pmums, :323-361 and :486-495):

  * rows with a -1 are dropped, the rest is ordered by column 0;
  * rank_j[i] = position of row i when the rows are ordered by column j; the pair (i, i + 1) is collinear when in every
    column both rows lie on the same strand and rank_j[i + 1] - rank_j[i] is +1 on '+' and -1 on '-';
  * with max_break > 0 the pair must also have max_j(|start_j[i] - start_j[i + 1]| - len_j) <= max_break, len_j the length
    of the row with the lower start;
  * a block is a maximal run of such pairs (first row, last row); with min_singleton_length = s every row in no block whose
    length is >= s is a block (i, i); blocks are numbered by their first row.

Equal starts in one column are ordered by row here (stable sorts); the reference leaves them to an unstable argsort, so
no test table has any among its kept rows (assert_no_ties).
"""
import numpy as np

NO_BLOCK = 0xFFFFFFFF


def prepare(lengths, starts, strands):
    """-> the filtered, sorted table (lengths u32 [n], starts i64 [n, N], strands bool [n, N])"""
    lengths = np.asarray(lengths, np.uint32)
    starts = np.asarray(starts, np.int64)
    if starts.ndim != 2:
        starts = starts.reshape(len(lengths), -1)
    strands = np.asarray(strands).astype(bool).reshape(starts.shape)
    keep = ~(starts == -1).any(axis=1)
    lengths, starts, strands = lengths[keep], starts[keep], strands[keep]
    if len(lengths) > 1 and not (np.diff(starts[:, 0]) >= 0).all():
        order = np.argsort(starts[:, 0], kind="stable")
        lengths, starts, strands = lengths[order], starts[order], strands[order]
    return lengths, starts, strands


def assert_no_ties(starts):
    starts = np.asarray(starts, np.int64)
    kept = starts[~(starts == -1).any(axis=1)]
    for j in range(kept.shape[1]):
        assert len(np.unique(kept[:, j])) == len(kept), "two kept rows share a start in column %d" % j


def good_pairs(lengths, starts, strands, max_break=1000):
    """bool [n - 1] over a prepared table: pair (i, i + 1) is collinear and within the gap limit"""
    n, N = starts.shape
    if n < 2:
        return np.zeros(0, bool)
    good = np.ones(n - 1, bool)
    gap = np.full(n - 1, np.iinfo(np.int64).min, np.int64)
    lens = lengths.astype(np.int64)
    for j in range(N):
        rank = np.empty(n, np.int64)
        rank[np.argsort(starts[:, j], kind="stable")] = np.arange(n)
        same = strands[:-1, j] == strands[1:, j]
        good &= same & (np.diff(rank) == np.where(strands[:-1, j], 1, -1))
        lower = np.where(starts[1:, j] < starts[:-1, j], lens[1:], lens[:-1])
        gap = np.maximum(gap, np.abs(starts[:-1, j] - starts[1:, j]) - lower)
    if max_break > 0:
        good &= gap <= max_break
    return good


def blocks(lengths, starts, strands, max_break=1000, min_singleton_length=None):
    """(n_blocks, 2) uint32 over a prepared table"""
    n = len(lengths)
    good = good_pairs(lengths, starts, strands, max_break)
    left = np.concatenate(([False], good))[:n] if n else np.zeros(0, bool)       # pair (i - 1, i)
    right = np.concatenate((good, [False]))[:n] if n else np.zeros(0, bool)      # pair (i, i + 1)
    single = np.zeros(n, bool)
    if min_singleton_length is not None and min_singleton_length >= 0:
        single = ~left & ~right & (lengths.astype(np.int64) >= min_singleton_length)
    first = np.nonzero((right & ~left) | single)[0]
    last = np.nonzero((left & ~right) | single)[0]
    return np.stack([first, last], axis=1).astype(np.uint32).reshape(-1, 2)


def row_blocks(blk, n):
    """u32 [n]: block of every row, NO_BLOCK for none"""
    out = np.full(n, NO_BLOCK, np.uint32)
    for b, (lo, hi) in enumerate(np.asarray(blk).reshape(-1, 2).tolist()):
        out[lo:hi + 1] = b
    return out


def mums_bytes(lengths, starts, strands, blk=None):
    """the .mums text of a table; with blk, the fourth field of every row"""
    rb = None if blk is None else row_blocks(blk, len(lengths))
    out = []
    for i, (length, row, srow) in enumerate(zip(lengths.tolist(), starts.tolist(), np.asarray(strands).tolist())):
        line = "%d\t%s\t%s" % (length, ",".join("" if x == -1 else str(x) for x in row),
                               ",".join(("+" if s else "-") if x != -1 else "" for s, x in zip(srow, row)))
        if rb is not None:
            line += "\t" + ("-" if rb[i] == NO_BLOCK else str(int(rb[i])))
        out.append(line + "\n")
    return "".join(out).encode()


def bumbl_bytes(lengths, starts, strands, blk=None):
    """the .bumbl bytes the reference's MUMdata.write_bums writes (utils.py:655-672): 32-bit lengths always"""
    lengths = np.ascontiguousarray(lengths, np.uint32)
    starts = np.ascontiguousarray(starts, np.int64).reshape(len(lengths), -1)
    flags = (1 << 15) | ((1 << 13) if (starts == -1).any() else 0) | ((1 << 14) if blk is not None else 0)
    out = [np.uint16(flags).tobytes(), np.uint64(starts.shape[1]).tobytes(), np.uint64(len(lengths)).tobytes(),
           lengths.tobytes(), starts.tobytes(), np.packbits(np.ascontiguousarray(strands, bool)).tobytes()]
    if blk is not None:
        blk = np.ascontiguousarray(blk, np.uint32).reshape(-1, 2)
        out += [np.uint64(len(blk)).tobytes(), blk.tobytes()]
    return b"".join(out)


# ---- seeded tables ---------------------------------------------------------------------------------------------------
def make_table(seed, n, n_docs, inversions=(), moves=(), minus_cols=(), partial=0, shuffle=False, base=0,
               gaps=(0, 120, 600, 1500), lengths=(20, 400), wide=()):
    """A syntenic table of n rows x n_docs columns with rearrangements, no two rows sharing a start in a column.

    Every column starts as the same chain: row i begins where row i - 1 ended plus a gap drawn from the ranges between
    consecutive `gaps` entries (so that limits of 200 and 1000 both cut somewhere).  inversions: (column, first, last) rows
    whose segment is reversed in place onto '-'; moves: (column, first, last) rows taken far behind the end of the column;
    minus_cols: whole columns reflected onto '-'; partial: that many cells set to -1 (rows to be dropped); shuffle: the rows
    are handed over in random order; base: added to every start (2^33: keys of 40 bits); wide: rows i with a gap of 1200 + i % 7
    in front of them in column i % n_docs (cuts at a limit of 1000 in tables whose `gaps` are all small)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lengths[0], lengths[1], n).astype(np.uint32)
    starts = np.zeros((n, n_docs), np.int64)
    strands = np.ones((n, n_docs), bool)
    for j in range(n_docs):
        kind = rng.integers(0, len(gaps) - 1, n)
        gap = rng.integers(np.asarray(gaps)[kind], np.asarray(gaps)[kind + 1])
        for i in wide:
            if i % n_docs == j:
                gap[i] = 1200 + i % 7
        pos = int(rng.integers(0, 5000))
        col = np.zeros(n, np.int64)
        for i in range(n):
            pos += int(gap[i])
            col[i] = pos
            pos += int(lens[i])
        starts[:, j] = col
    end = int((starts + lens[:, None].astype(np.int64)).max()) + 10000 if n else 0
    for j, a, b in inversions:              # rows a..b of column j, reversed in place
        lo, hi = int(starts[a, j]), int(starts[b, j] + lens[b])
        starts[a:b + 1, j] = lo + hi - (starts[a:b + 1, j] + lens[a:b + 1])
        strands[a:b + 1, j] = False
    for k, (j, a, b) in enumerate(moves):   # rows a..b of column j, far away
        starts[a:b + 1, j] += end * (k + 1)
    for j in minus_cols:
        top = int((starts[:, j] + lens).max())
        starts[:, j] = top - (starts[:, j] + lens)
        strands[:, j] = ~strands[:, j]
    starts += base
    if partial:
        rows = rng.choice(n, size=min(partial, n), replace=False)
        cols = rng.integers(0, n_docs, len(rows))
        starts[rows, cols] = -1
        strands[rows, cols] = False
    if shuffle:
        order = rng.permutation(n)
        lens, starts, strands = lens[order], starts[order], strands[order]
    assert_no_ties(starts)
    return lens, starts, strands
