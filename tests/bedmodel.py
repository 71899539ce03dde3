"""Host model of the BED writer (`mumemto bed`, mumemto/mum_to_bed.py), in closed form (numpy).

For column c of a table, min_singleton_length L and the contigs (name_k, len_k) of the sequence:

  * with blocks (first, last): one record per block and one per row in no block with length >= L; without: one per row with a
    start in c and length >= L; in ascending order of the first row;
  * a block is [start[first], start[last] + length[last]) when its LAST row is on '+' in c, [start[last], start[first] +
    length[first]) otherwise; a row is [start, start + length); the strand is that of the last row;
  * name = the block's number, or -1 - i for a row: i = the rank of the row among the rows with a start in c;
  * ends_k = len_0 + ... + len_k; the contig is the first k with ends_k > begin (searchsorted, side='right'); a begin at or
    beyond the total gets the last contig (counted: clamped); rel_start = begin - (ends_k - len_k), rel_end = rel_start +
    (end - begin);
  * the line: name_k <TAB> rel_start <TAB> rel_end <TAB> block_<b> | mum_<i> <TAB> + | - <NL>.

drop_open_tail=True reproduces the reference, which never flushes a block that ends the table: its record is missing there.
"""
import numpy as np

NO_BLOCK = 0xFFFFFFFF
FIELDS = 5


def row_blocks(blocks, n):
    out = np.full(n, NO_BLOCK, np.int64)
    for b, (lo, hi) in enumerate(np.asarray(blocks, np.int64).reshape(-1, 2).tolist()):
        out[lo:hi + 1] = b
    return out


def intervals(lengths, starts, strands, col, min_single=100, blocks=None, drop_open_tail=False):
    """-> (begin, end, name, strand) int64 [k] each, the records of column col in order"""
    lengths = np.asarray(lengths, np.int64)
    s = np.asarray(starts, np.int64).reshape(len(lengths), -1)[:, col]
    plus_of = np.asarray(strands).astype(bool).reshape(len(lengths), -1)[:, col]
    n = len(lengths)
    rows = np.arange(n, dtype=np.int64)
    if blocks is not None:
        blocks = np.asarray(blocks, np.int64).reshape(-1, 2)
        rb = row_blocks(blocks, n)
        free = rb == NO_BLOCK
        head = np.zeros(n, bool)
        head[blocks[:, 0]] = True
        flag = head | (free & (lengths >= min_single))
        if drop_open_tail and n and not free[-1]:
            flag[blocks[rb[-1], 0]] = False
        first = rows[flag]
        b = rb[first]
        last = np.where(b == NO_BLOCK, first, blocks[np.where(b == NO_BLOCK, 0, b), 1] if len(blocks) else first)
        name = np.where(b == NO_BLOCK, -1 - first, b)
    else:
        present = s != -1
        flag = present & (lengths >= min_single)
        first = last = rows[flag]
        name = -1 - (np.cumsum(present) - present)[flag]
    plus = plus_of[last]
    begin = np.where(plus, s[first], s[last])
    end = np.where(plus, s[last] + lengths[last], s[first] + lengths[first])
    return begin, end, name.astype(np.int64), plus.astype(np.int64)


def lookup(begin, contig_lens):
    """-> (contig, rel_start, clamped mask)"""
    lens = np.asarray(contig_lens, np.int64)
    ends = np.cumsum(lens)
    k = np.searchsorted(ends, begin, side="right")
    clamped = k >= len(ends)
    k = np.minimum(k, len(ends) - 1)
    return k.astype(np.int64), begin - (ends - lens)[k], clamped


def records_of(lengths, starts, strands, col, contig_lens, min_single=100, blocks=None, drop_open_tail=False):
    """-> (records int64 [k, 5] = (contig, rel_start, rel_end, name, strand), number of clamped records)"""
    begin, end, name, plus = intervals(lengths, starts, strands, col, min_single, blocks, drop_open_tail)
    k, rel, clamped = lookup(begin, contig_lens)
    return np.stack([k, rel, rel + (end - begin), name, plus], axis=1).reshape(-1, FIELDS), int(clamped.sum())


def bed(lengths, starts, strands, contigs, seq_idx=None, min_single=100, blocks=None):
    """what Merged.bed leaves: (record_begin uint64 [n_docs + 1], records int64 [n, 5], clamped)"""
    n_docs = np.asarray(starts).reshape(len(lengths), -1).shape[1] if len(lengths) else len(contigs[1])
    cols = range(n_docs) if seq_idx is None else [seq_idx]
    record_begin = np.zeros(n_docs + 1, np.uint64)
    parts, clamped, at = [], 0, 0
    for c in range(n_docs):
        record_begin[c] = at
        if c in cols and len(lengths):
            rec, cl = records_of(lengths, starts, strands, c, contigs[1][c], min_single, blocks)
            parts.append(rec)
            clamped += cl
            at += len(rec)
    record_begin[n_docs] = at
    return record_begin, (np.concatenate(parts) if parts else np.zeros((0, FIELDS), np.int64)).reshape(-1, FIELDS), clamped


def label(name):
    return "block_%d" % name if name >= 0 else "mum_%d" % (-1 - name)


def text(records, names):
    """the bytes of the lines of one column's records; names: the contig names of that column"""
    return "".join("%s\t%d\t%d\t%s\t%s\n" % (names[k], a, b, label(nm), "+" if st else "-")
                   for k, a, b, nm, st in np.asarray(records, np.int64).reshape(-1, FIELDS).tolist()).encode()


def bed_bytes(lengths, starts, strands, col, contigs, min_single=100, blocks=None, drop_open_tail=False):
    rec, _ = records_of(lengths, starts, strands, col, contigs[1][col], min_single, blocks, drop_open_tail)
    return text(rec, contigs[0][col])


def ends_in_block(blocks, n):
    return blocks is not None and len(blocks) > 0 and int(np.asarray(blocks).reshape(-1, 2)[-1, 1]) == n - 1


# ---- seeded inputs --------------------------------------------------------------------------------------------------------
def make_contigs(seed, totals, counts, name_len=(1, 12), zero=0.0):
    """(names, lengths) for sequences of the given totals: counts[c] contigs each, a share `zero` of them of length 0"""
    rng = np.random.default_rng(seed)
    names, lengths = [], []
    for c, (total, cnt) in enumerate(zip(totals, counts)):
        w = rng.integers(1, 1000, cnt).astype(np.float64)
        w[rng.random(cnt) < zero] = 0
        if not w.any():
            w[-1] = 1
        lens = np.floor(w / w.sum() * int(total)).astype(np.int64)
        lens[np.nonzero(w)[0][-1]] += int(total) - int(lens.sum())
        names.append(["s%dc%d_%s" % (c, k, "x" * int(rng.integers(*name_len))) for k in range(cnt)])
        lengths.append(lens.tolist())
    return names, lengths


def make_rows(seed, n, n_docs, absent=0.0, base=0, lengths=(20, 400)):
    """n rows, starts ascending in every column (a step of 0-2000 beyond the row before), strands random; a share `absent` of the
    cells is -1.  -> (lengths u32, starts i64, strands bool, totals: the end of the last row of every column + 1)"""
    rng = np.random.default_rng(seed)
    L = rng.integers(lengths[0], lengths[1], n).astype(np.uint32)
    step = rng.integers(0, 2000, (n, n_docs)) + L.astype(np.int64)[:, None]
    s = base + np.cumsum(step, axis=0) - step
    totals = (s[-1] + L[-1] + 1).tolist() if n else [1] * n_docs
    st = rng.random((n, n_docs)) < 0.5
    if absent:
        s = np.where(rng.random((n, n_docs)) < absent, -1, s)
    return L, s.astype(np.int64), st, totals


def make_blocks(seed, n, share=0.6, max_len=9, one_row=True):
    """an ascending, disjoint block list over n rows (first, last), one-row blocks among them"""
    rng = np.random.default_rng(seed)
    out, r = [], 0
    while r < n:
        if rng.random() < share:
            k = int(rng.integers(1 if one_row else 2, max_len))
            last = min(n - 1, r + k - 1)
            if last > r or one_row:
                out.append((r, last))
            r = last + 1
        else:
            r += 1
    return np.asarray(out, np.uint32).reshape(-1, 2)
