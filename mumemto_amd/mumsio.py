"""PREFIX.mums / PREFIX.bumbl tables as NumPy arrays (host-side I/O for the merge tools), and PREFIX.mems rows in batches.

Formats as the reference reads and writes them (mumemto/utils.py:69-87,627-632,655-665; include/mumsio.hpp:105-194):
  .mums   one row per line: `length <TAB> off_0,off_1,... <TAB> s_0,s_1,...` (empty offset = absent, strands + / -),
          after `mumemto collinear` a fourth field: the number of the row's collinear block, or `-`
  .bumbl  u16 flags (bit 13 partial, bit 14 collinear blocks, bit 15 32-bit lengths) | u64 n_docs | u64 n_rows |
          lengths (u16 or u32) | offsets i64 [n_rows][n_docs] | strand bits, row-major, most significant bit first |
          with bit 14: u64 n_blocks | n_blocks x (u32 first row, u32 last row)
  .mems   one row per line: `length <TAB> start,start,... <TAB> doc,doc,... <TAB> strand,strand,...`, one entry per occurrence
          (read_mems; the reference reads them in mumemto/mem_density.py:31-36)
"""
import numpy as np

FLAG_PARTIAL = 1 << 13
FLAG_BLOCKS = 1 << 14
FLAG_LENGTH32 = 1 << 15
NO_BLOCK = 0xFFFFFFFF


def read_mums(path, with_blocks=False):
    """-> (lengths u32 [n], starts i64 [n, N] with -1 = absent, strands bool [n, N]); a fourth field (the row's collinear
    block) is tolerated, and with_blocks=True returned as a fourth item: u32 [n] with NO_BLOCK for `-` (and for `*`, the
    reference's other spelling of "none"), or None when no row carries one.  Fields beyond the fourth are ignored here."""
    lengths, starts, strands, blocks = [], [], [], []
    with open(path, "rb") as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            lengths.append(int(parts[0]))
            starts.append([int(x) if x else -1 for x in parts[1].split(b",")])
            strands.append([x == b"+" for x in parts[2].split(b",")])
            if len(parts) > 3:
                blocks.append(NO_BLOCK if parts[3] in (b"-", b"*") else int(parts[3]))
    n_docs = len(starts[0]) if starts else 0
    rows = (np.array(lengths, np.uint32), np.array(starts, np.int64).reshape(len(lengths), n_docs),
            np.array(strands, bool).reshape(len(lengths), n_docs))
    if not with_blocks:
        return rows
    if blocks and len(blocks) != len(lengths):
        raise ValueError("%s: only some rows carry a block field" % path)
    return rows + (np.array(blocks, np.uint32) if blocks else None,)


def mums_extra_fields(path):
    """the largest number of tab- or space-separated fields on a line of a .mums file"""
    with open(path, "rb") as f:
        return max((len(line.split()) for line in f), default=0)


def read_bumbl(path, with_blocks=False):
    """-> (lengths, starts, strands); with_blocks=True also the block list u32 [n_blocks, 2] (first row, last row), or None
    when the header does not announce one"""
    raw = np.fromfile(path, np.uint8)
    flags = int(raw[:2].view(np.uint16)[0])
    n_docs, n_rows = (int(x) for x in raw[2:18].view(np.uint64))
    pos = 18
    if flags & FLAG_LENGTH32:
        lengths = raw[pos:pos + 4 * n_rows].view(np.uint32).copy()
        pos += 4 * n_rows
    else:
        lengths = raw[pos:pos + 2 * n_rows].view(np.uint16).astype(np.uint32)
        pos += 2 * n_rows
    cells = n_rows * n_docs
    starts = raw[pos:pos + 8 * cells].view(np.int64).reshape(n_rows, n_docs).copy()
    pos += 8 * cells
    bits = np.unpackbits(raw[pos:pos + (cells + 7) // 8])[:cells]
    rows = (lengths, starts, bits.astype(bool).reshape(n_rows, n_docs))
    if not with_blocks:
        return rows
    pos += (cells + 7) // 8
    blocks = None
    if flags & FLAG_BLOCKS:
        n_blocks = int(raw[pos:pos + 8].view(np.uint64)[0])
        blocks = raw[pos + 8:pos + 8 + 8 * n_blocks].view(np.uint32).reshape(n_blocks, 2).copy()
    return rows + (blocks,)


def read_rows(path):
    return read_bumbl(path) if path.endswith(".bumbl") else read_mums(path)


def write_mums(path, lengths, starts, strands, row_block=None):
    """row_block: u32 [n], the collinear block of every row (NO_BLOCK: `-`), written as a fourth field"""
    with open(path, "w") as f:
        if row_block is None:
            for length, row, srow in zip(lengths.tolist(), starts.tolist(), strands.tolist()):
                f.write("%d\t%s\t%s\n" % (length, ",".join(map(str, row)), ",".join("+" if s else "-" for s in srow)))
            return
        for length, row, srow, b in zip(lengths.tolist(), starts.tolist(), strands.tolist(), np.asarray(row_block).tolist()):
            f.write("%d\t%s\t%s\t%s\n" % (length, ",".join(map(str, row)), ",".join("+" if s else "-" for s in srow),
                                          "-" if b == NO_BLOCK else b))


def write_bumbl(path, lengths, starts, strands, blocks=None):
    """blocks: u32 [n_blocks, 2] (first row, last row) -- sets header bit 14 and follows the strand bits"""
    lengths = np.ascontiguousarray(lengths)
    starts = np.ascontiguousarray(starts, np.int64)
    flags = (FLAG_PARTIAL if (starts == -1).any() else 0) | (FLAG_LENGTH32 if lengths.dtype == np.uint32 else 0)
    flags |= FLAG_BLOCKS if blocks is not None else 0
    with open(path, "wb") as f:
        f.write(np.uint16(flags).tobytes())
        f.write(np.uint64(starts.shape[1] if starts.ndim == 2 else 0).tobytes())
        f.write(np.uint64(len(lengths)).tobytes())
        f.write(lengths.tobytes())
        f.write(starts.tobytes())
        f.write(np.packbits(np.ascontiguousarray(strands, bool)).tobytes())
        if blocks is not None:
            blocks = np.ascontiguousarray(blocks, np.uint32).reshape(-1, 2)
            f.write(np.uint64(len(blocks)).tobytes())
            f.write(blocks.tobytes())


def _ints_by_row(fields, path, line_numbers, what):
    """The comma-separated integers of one field of many rows, parsed by numpy over the bytes of all rows at once: ->
    (values int64 [T], count per row int64 [n]).  Digits are weighted by their power of ten and summed per token."""
    buf = np.frombuffer(b";".join(fields), np.uint8)
    comma, semi = buf == 0x2C, buf == 0x3B
    sep = comma | semi
    at = np.nonzero(sep)[0]
    ends = np.concatenate((at, [len(buf)]))                      # one token ends before every separator, and at the end
    begins = np.concatenate(([0], at + 1))
    row_end = np.concatenate((semi[at], [True]))                 # the token is the last of its row
    counts = np.diff(np.concatenate(([-1], np.nonzero(row_end)[0])))
    if len(counts) != len(fields):
        raise ValueError("%s, lines %d-%d: a `;` in field %s" % (path, line_numbers[0], line_numbers[-1], what))
    neg = np.zeros(len(begins), bool)
    inside = begins < len(buf)
    neg[inside] = buf[begins[inside]] == 0x2D
    digit = buf.astype(np.int64) - 48
    is_digit = (digit >= 0) & (digit <= 9)
    sign_at = np.zeros(len(buf), bool)
    sign_at[begins[neg]] = True
    n_digits = ends - begins - neg
    bad = (n_digits < 1) | (n_digits > 18)
    if bad.any() or not (is_digit | sep | sign_at).all():
        t = int(np.nonzero(bad)[0][0]) if bad.any() else int(np.cumsum(sep)[np.nonzero(~(is_digit | sep | sign_at))[0][0]])
        row = int(np.searchsorted(np.cumsum(counts), t, side="right"))
        raise ValueError("%s, line %d: field %s holds something that is no integer" % (path, line_numbers[row], what))
    token = np.cumsum(sep)                                       # the token of every byte (of a separator: the one behind it)
    power = ends[token] - 1 - np.arange(len(buf))
    weighted = np.where(is_digit, digit * 10 ** np.clip(power, 0, 18), 0)
    values = np.add.reduceat(weighted, begins[inside]) if len(buf) else np.zeros(0, np.int64)
    return np.where(neg[inside], -values, values).astype(np.int64), counts


def read_mems(path, max_occ=1 << 24):
    """A PREFIX.mems file (one row per line: `length <TAB> start,start,... <TAB> doc,doc,... <TAB> strand,...`, one entry per
    occurrence) as a generator of batches of whole rows: (lengths u32 [n], occ_start u64 [n + 1] from 0, starts i64 [T],
    docs u64 [T]).  A batch holds at most max_occ occurrences unless a single row has more; batches keep the order of the file.
    Strands are not read: the density has no use for them.  Beyond splitting the lines all parsing is numpy's, over the bytes
    of many rows at once.

    One departure from the reference (mumemto/mem_density.py zips the two fields and silently drops the tail of the longer
    one): a line whose second and third fields differ in count is refused, ValueError with its line number.  So are a line
    with fewer than three fields, a field that holds something other than integers, a negative length or document."""
    max_occ = max(int(max_occ), 1)
    line_no = 0
    with open(path, "rb") as f:
        while True:
            lines = f.readlines(max(1 << 16, 16 * max_occ))          # whole lines, about that many bytes
            if not lines:
                return
            rows = [(line_no + k + 1, fields) for k, fields in enumerate(l.split() for l in lines) if fields]
            line_no += len(lines)
            if not rows:
                continue
            numbers = [no for no, _ in rows]
            short = [no for no, fields in rows if len(fields) < 3]
            if short:
                raise ValueError("%s, line %d: fewer than three fields (length, starts, documents)" % (path, short[0]))
            lengths, _ = _ints_by_row([fields[0] for _, fields in rows], path, numbers, "1 (the length)")
            starts, n_starts = _ints_by_row([fields[1] for _, fields in rows], path, numbers, "2 (the starts)")
            docs, n_docs = _ints_by_row([fields[2] for _, fields in rows], path, numbers, "3 (the documents)")
            if len(lengths) != len(rows):
                raise ValueError("%s, line %d: field 1 holds more than the length" % (path, numbers[0]))
            differ = np.nonzero(n_starts != n_docs)[0]
            if len(differ):
                r = int(differ[0])
                raise ValueError("%s, line %d: %d starts but %d documents" % (path, numbers[r], int(n_starts[r]), int(n_docs[r])))
            if (lengths < 0).any() or (lengths >> 32).any() or (docs < 0).any():
                r = int(np.nonzero((lengths < 0) | (lengths >> 32 != 0))[0][0]) if ((lengths < 0) | (lengths >> 32 != 0)).any() \
                    else int(np.searchsorted(np.cumsum(n_docs), np.nonzero(docs < 0)[0][0], side="right"))
                raise ValueError("%s, line %d: a length outside [0, 2^32) or a negative document" % (path, numbers[r]))
            occ_start = np.concatenate(([0], np.cumsum(n_starts)))
            r0 = 0
            while r0 < len(rows):                                     # one turn per batch
                r1 = int(np.searchsorted(occ_start, occ_start[r0] + max_occ, side="right")) - 1
                r1 = min(max(r1, r0 + 1), len(rows))
                i, j = int(occ_start[r0]), int(occ_start[r1])
                yield (lengths[r0:r1].astype(np.uint32), (occ_start[r0:r1 + 1] - occ_start[r0]).astype(np.uint64),
                       starts[i:j], docs[i:j].astype(np.uint64))
                r0 = r1


def read_seq_lengths(path):
    """the length of every sequence of a PREFIX.lengths file, as the reference's get_sequence_lengths reads it
    (mumemto/utils.py:177-207): the second field of every line, or, of a multi-FASTA file (`PATH * total` followed by the
    `PATH name length` lines of the contigs), the sum of the third fields of a sequence's contig lines"""
    lines = [l.split() for l in open(path).read().splitlines()]
    if not (lines and len(lines[0]) > 1 and lines[0][1] == "*"):
        return [int(l[1]) for l in lines]
    out, cur = [], []
    for l in lines:
        if l[1] == "*":
            if cur:
                out.append(cur)
            cur = []
            continue
        cur.append(int(l[2]))
    out.append(cur)
    return [sum(o) for o in out]


def read_contigs(path):
    """(names, lengths) of the contigs of a multi-FASTA PREFIX.lengths file, one list per sequence in file order, from the lines
    the reference's get_sequence_lengths(multilengths=True) and get_contig_names read (mumemto/utils.py:180-192,221-247): a
    `PATH * total` line begins a sequence, the `PATH name length` lines behind it are its contigs.  As there, a `*` line
    directly behind another one begins no sequence of its own.  A plain `PATH length` file is refused: it has no contigs."""
    lines = [l.split() for l in open(path).read().splitlines()]
    if not (lines and len(lines[0]) > 1 and lines[0][1] == "*"):
        raise ValueError("%s has no contig lines: the lengths file must come from a multi-FASTA-aware run "
                         "(`PATH * total` lines followed by `PATH name length` lines)" % path)
    names, lengths, cur_n, cur_l = [], [], [], []
    for l in lines:
        if l[1] == "*":
            if cur_n:
                names.append(cur_n)
                lengths.append(cur_l)
            cur_n, cur_l = [], []
            continue
        cur_n.append(l[1])
        cur_l.append(int(l[2]))
    names.append(cur_n)
    lengths.append(cur_l)
    return names, lengths
