"""Plain-Python model of the multi-MUM sequence writer (csrc/sequences.cpp), written line by line from the reference's two
forms: the binary src/extract_mums.cpp (`BINARY`) and the user tool mumemto/extract_mums.py (`PYTHON`).

BINARY (extract_mums.cpp:98-112): for every row of the file, in its order,
    `>mum_<count>\\n`, ref_seq.substr(first, length), `#` with the terminator, `\\n`
substr cuts at the end of the string, gives "" for a start at the end, and throws for a start beyond it; a row without a start
in the first document makes the tool exit 1 (partial MUMs).  Strands are not looked at; the bytes are the file's.

PYTHON (extract_mums.py:47-56): for every row
    `>mum_<i>`, then seq[start : start + length].upper(), reverse-complemented when the row is on `-`, and `#`
and the lines joined by `\\n`.  The slice cuts at the end and gives "" for a start at or beyond it; a start of -1 gives
seq[-1 : length - 1], which is "" for every length up to the sequence's -- that case is the rule here: an empty record.

The complement is Biopython's in the reference, which is not available here; the table below is the one this project decided
(csrc/sequence_kernels.hip): A<->T, C<->G, M<->K, R<->Y, V<->B, H<->D; W, S, N, X and every other byte stay.
"""
BINARY, PYTHON = "binary", "python"

COMPLEMENT = bytes.maketrans(b"ATCGMKRYVBHD", b"TAGCKMYRBVDH")
UPPER = bytes.maketrans(bytes(range(ord("a"), ord("z") + 1)), bytes(range(ord("A"), ord("Z") + 1)))


class Refused(ValueError):
    """what the library refuses with std::invalid_argument; .kind is one of: column, start, partial, beyond"""

    def __init__(self, kind, row=None):
        ValueError.__init__(self, "%s (row %s)" % (kind, row))
        self.kind, self.row = kind, row


def reverse_complement(seq):
    return seq[::-1].translate(COMPLEMENT)


def record_bases(seq, start, length, plus, dialect):
    """the bases of one record; None where the dialect refuses the row"""
    n = len(seq)
    if start == -1 or start > n:
        return None if dialect == BINARY else b""
    cur = seq[start:start + length]                       # cut at the end; "" at the end
    if dialect == BINARY:
        return cur
    cur = cur.translate(UPPER)
    return cur if plus else reverse_complement(cur)


def sequences(seq, lengths, starts, strands, col, dialect=PYTHON, terminator=True):
    """seq: the bases of document col (bytes); lengths [n], starts [n][N], strands [n][N] (true = '+') -> the text (bytes).
    The refusals are looked for in the library's order: the column; over all rows a start below -1; then a row without a
    start; then a start beyond the end -- each naming the first such row."""
    n_docs = len(starts[0]) if len(starts) else None
    if n_docs is not None and not 0 <= col < n_docs:
        raise Refused("column")
    rows = [(int(lengths[i]), int(starts[i][col]), bool(strands[i][col])) for i in range(len(lengths))]
    for i, (_, s, _) in enumerate(rows):
        if s < -1:
            raise Refused("start", i)
    if dialect == BINARY:
        for kind, bad in (("partial", lambda s: s == -1), ("beyond", lambda s: s > len(seq))):
            for i, (_, s, _) in enumerate(rows):
                if bad(s):
                    raise Refused(kind, i)
    term = b"#" if terminator else b""
    records = [b">mum_%d\n" % i + record_bases(seq, s, length, plus, dialect) + term for i, (length, s, plus) in enumerate(rows)]
    if dialect == BINARY:
        return b"".join(r + b"\n" for r in records)
    return b"\n".join(records)


def stats(seq, lengths, starts, col, dialect=PYTHON):
    """(records, bases written, rows cut at the end, empty records) of a text that is not refused"""
    n, bases, clipped, empty = len(seq), 0, 0, 0
    for length, row in zip(lengths, starts):
        s = int(row[col])
        nb = 0 if s == -1 or s > n else min(int(length), n - s)
        bases += nb
        clipped += 0 <= s <= n and nb < int(length)
        empty += nb == 0
    return len(lengths), bases, clipped, empty


def read_fasta(path):
    """the bases of a FASTA file, records concatenated (what kseq gives the binary and the line filter gives the Python tool)"""
    import gzip
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return b"".join(l.strip() for l in raw.splitlines() if not l.startswith(b">"))
