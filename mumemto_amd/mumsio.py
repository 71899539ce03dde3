"""PREFIX.mums / PREFIX.bumbl tables as NumPy arrays (host-side I/O for the merge tools).

Formats as the reference reads and writes them (mumemto/utils.py:69-87,627-632,655-665; include/mumsio.hpp:105-194):
  .mums   one row per line: `length <TAB> off_0,off_1,... <TAB> s_0,s_1,...` (empty offset = absent, strands + / -),
          after `mumemto collinear` a fourth field: the number of the row's collinear block, or `-`
  .bumbl  u16 flags (bit 13 partial, bit 14 collinear blocks, bit 15 32-bit lengths) | u64 n_docs | u64 n_rows |
          lengths (u16 or u32) | offsets i64 [n_rows][n_docs] | strand bits, row-major, most significant bit first |
          with bit 14: u64 n_blocks | n_blocks x (u32 first row, u32 last row)
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
