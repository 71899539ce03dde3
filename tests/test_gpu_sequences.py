"""GPU: the multi-MUM sequence writer (csrc/sequences.cpp, sequence_kernels.hip) against the files the reference's extract_mums
binary wrote (tests/golden/string_merge) and against the host model tests/seqmodel.py, which tests/test_sequences_host.py holds
to the same files and to hand-written rows.  Every comparison is exact, byte for byte."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import seqmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "string_merge")
CASES = sorted(os.listdir(GOLD))
PARTS = sorted(p[: -len("_mums.fa")] for p in glob.glob(os.path.join(GOLD, "*", "p*_mums.fa")))
PART_IDS = ["/".join(p.split(os.sep)[-2:]) for p in PARTS]
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
TOOL = [sys.executable, "-m", "mumemto_amd.extract_mums"]
DIALECTS = (M.BINARY, M.PYTHON)


def kernel_constant(name):
    text = open(os.path.join(ROOT, "mumemto_amd", "csrc", "sequence_kernels.hpp")).read()
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))


CHUNK, BLOCK, ITEMS, LDS_RECORDS = (kernel_constant(k) for k in ("CHUNK", "FORMAT_BLOCK", "FORMAT_ITEMS", "LDS_RECORDS"))
TILE_BYTES = CHUNK * BLOCK * ITEMS
assert (CHUNK, TILE_BYTES, LDS_RECORDS) == (16, 16384, 1024)


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def random_document(n, seed, plain=False):
    """mixed case, N and IUPAC codes among the bases (plain: A C G T alone)"""
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).astype(np.uint8)
    if not plain:
        for p in rng.integers(0, n, size=max(n // 50, 4)):
            seq[p] = rng.choice(np.frombuffer(b"acgtNnRYKMSWBDHVXx", np.uint8))
        a = int(rng.integers(0, max(n - 300, 1)))
        seq[a:a + 70] = ord("N")
        seq[a + 100:a + 180] = np.frombuffer(seq[a + 100:a + 180].tobytes().lower(), np.uint8)
    return seq.tobytes()


def one_column(lengths, starts, plus, n_docs=3, col=1):
    """a table of n_docs columns whose column col is the one given; the others hold rows that would be refused"""
    n = len(lengths)
    table_starts = np.full((n, n_docs), -1, np.int64)
    table_starts[:, col] = starts
    table_strands = np.ones((n, n_docs), bool)
    table_strands[:, col] = plus
    return np.asarray(lengths, np.uint32), table_starts, table_strands


def compare(engine, seq, table, col, dialects=DIALECTS, terminators=(True, False), path=None):
    """the device's text for every dialect and terminator against the model; -> the stats of the last one"""
    import mumemto_amd
    stats = None
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        for dialect in dialects:
            for term in terminators:
                want = M.sequences(seq, *table, col, dialect, term)
                k = m.sequences(col, seq, dialect, term)
                got = m.sequences_text()
                assert k == len(want) == len(got)
                assert got == want, (dialect, term, first_difference(got, want))
                offsets = m.sequences_offsets()
                assert offsets[0] == 0 and offsets[-1] == len(want)
                heads = [want.index(b">mum_%d\n" % i, int(offsets[i])) == int(offsets[i]) for i in range(0, len(table[0]), max(len(table[0]) // 50, 1))]
                assert all(heads)
                stats = m.sequences_stats()
                assert (stats["records"], stats["bases"], stats["clipped"], stats["empty"]) == M.stats(seq, table[0], table[1], col, dialect)
                assert stats["text_bytes"] == len(want)
                if path is not None:
                    m.write_sequences(path)
                    assert read(path) == want and not os.path.exists(path + ".tmp")
                    stats = m.sequences_stats()
    return stats


def first_difference(a, b):
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return i, a[max(i - 20, 0):i + 20], b[max(i - 20, 0):i + 20]


# ---- 1. the golden cases: through the ABI, the tool, and the merge driver -----------------------------------------------------------
@pytest.mark.parametrize("prefix", PARTS, ids=PART_IDS)
def test_golden_through_the_abi(engine, prefix, tmp_path):
    import mumemto_amd
    from mumemto_amd import mumsio
    table = mumsio.read_mums(prefix + ".mums")
    fasta = os.path.join(os.path.dirname(prefix), read(prefix + ".lengths").split()[0].decode())
    want = read(prefix + "_mums.fa")
    out = str(tmp_path / "out.fa")
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        assert m.sequences(0, fasta, "binary") == len(want)                   # the FASTA file read by the library
        assert m.sequences_text() == want
        m.write_sequences(out)
        assert read(out) == want and os.listdir(str(tmp_path)) == ["out.fa"]
        assert m.sequences(0, M.read_fasta(fasta), "binary", False) == len(want) - len(table[0])     # the bases handed over
        assert m.sequences_text() == want.replace(b"#\n", b"\n")
    assert mumemto_amd.extract_mums(*table, fasta, 0, "binary") == want


@pytest.mark.parametrize("prefix", PARTS, ids=PART_IDS)
def test_golden_through_the_tool(prefix, tmp_path):
    work = str(tmp_path / "case")
    shutil.copytree(os.path.dirname(prefix), work)
    name = os.path.basename(prefix)
    os.remove(os.path.join(work, name + "_mums.fa"))
    r = subprocess.run(TOOL + ["-m", name + ".mums", "--dialect", "binary"], cwd=work, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert read(os.path.join(work, name + "_mums.fa")) == read(prefix + "_mums.fa")       # the default output name
    assert not [f for f in os.listdir(work) if f.endswith(".tmp")]


@pytest.mark.parametrize("case", CASES)
def test_golden_through_the_merge_driver(case, tmp_path, monkeypatch):
    from mumemto_amd import merge_mums
    work = str(tmp_path / case)
    shutil.copytree(os.path.join(GOLD, case), work)
    parts = sorted(os.path.basename(p) for p in PARTS if os.path.dirname(p) == os.path.join(GOLD, case))
    for p in parts:
        os.remove(os.path.join(work, p + "_mums.fa"))
    cwd = os.getcwd()
    os.chdir(work)
    monkeypatch.setenv("MUMEMTO_NO_TORCH", "1")              # (the children need no tensor library: a quicker start)
    try:
        args = merge_mums.parse_arguments([p + ".mums" for p in parts] + ["-o", "ours", "--extract-on-device"])
        merge_mums.run_merger(args)                          # step 1 on the device, step 2 as ever
        for p in parts:
            assert read(p + "_mums.fa") == read(os.path.join(GOLD, case, p + "_mums.fa")), p
        assert os.path.getsize("ours_temp_merged.mums") > 0
    finally:
        os.chdir(cwd)


def test_tool_python_dialect_and_the_length_check(tmp_path):
    """the tool's defaults are the PYTHON dialect; a sequence whose length is not the lengths file's is an error, exit 1"""
    from mumemto_amd import mumsio
    seq = random_document(5000, 3)
    lengths = np.array([30, 17, 64, 9], np.uint32)
    starts = np.array([[10, 4000], [-1, 33], [200, 4990], [77, 5000]], np.int64)
    strands = np.array([[True, False], [True, True], [False, False], [True, False]])
    other = random_document(700, 4, plain=True)
    with open(str(tmp_path / "a.fa"), "wb") as f:
        f.write(b">a\n" + other + b"\n")
    with open(str(tmp_path / "b.fa"), "wb") as f:
        f.write(b">r0 x\n" + seq[:1234] + b"\n>r1\n" + seq[1234:3000] + b"\n" + seq[3000:] + b"\n")     # two records, a broken line
    mumsio.write_mums(str(tmp_path / "t.mums"), lengths, starts, strands)
    mumsio.write_bumbl(str(tmp_path / "t.bumbl"), lengths, starts, strands)
    (tmp_path / "t.lengths").write_text("%s 700\n%s 5000\n" % (tmp_path / "a.fa", tmp_path / "b.fa"))
    for table, out, extra in (("t.mums", "x", []), ("t.bumbl", "y.fasta", ["-t", "-v"])):
        r = subprocess.run(TOOL + ["-m", str(tmp_path / table), "-i", "1", "-o", str(tmp_path / out)] + extra, cwd=ROOT,
                           capture_output=True, timeout=120, env=CHILD_ENV)
        assert r.returncode == 0 and r.stdout == b"", r.stderr
        name = out if out.endswith(".fasta") else out + ".fa"
        assert read(str(tmp_path / name)) == M.sequences(seq, lengths, starts, strands, 1, M.PYTHON, not extra)
    (tmp_path / "t.lengths").write_text("%s 700\n%s 4999\n" % (tmp_path / "a.fa", tmp_path / "b.fa"))
    r = subprocess.run(TOOL + ["-m", str(tmp_path / "t.mums"), "-i", "1", "-o", str(tmp_path / "z")], cwd=ROOT, capture_output=True,
                       timeout=120, env=CHILD_ENV)
    assert r.returncode == 1 and not os.path.exists(str(tmp_path / "z.fa")) and not os.path.exists(str(tmp_path / "z.fa.tmp"))
    assert b"Sequence length 5000 does not match expected length 4999. There may be Ns or other non-ACGT chars" in r.stderr
    # the binary dialect refuses the partial row, like the binary
    r = subprocess.run(TOOL + ["-m", str(tmp_path / "t.mums"), "--dialect", "binary", "-o", str(tmp_path / "w")], cwd=ROOT,
                       capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 1 and b"row 1 has no start in column 0" in r.stderr and not os.path.exists(str(tmp_path / "w.fa"))


# ---- 2 - 6. the shapes the kernel can go wrong at ------------------------------------------------------------------------------------
def test_record_lengths_0_1_15_16_17(engine):
    """several records inside one 16-byte chunk, records that straddle chunks, on both strands"""
    seq = random_document(3000, 5)
    rng = np.random.default_rng(6)
    lengths = np.array([0, 1, 15, 16, 17] * 60 + [0] * 9 + [1] * 9, np.uint32)
    rng.shuffle(lengths[:300])
    starts = rng.integers(0, 2900, size=len(lengths))
    compare(engine, seq, one_column(lengths, starts, rng.integers(0, 2, size=len(lengths)).astype(bool)), 1)


@pytest.mark.parametrize("n", [11, 101, 1001, 1100])
def test_row_indices_change_width_inside_a_tile(engine, n):
    """9 -> 10, 99 -> 100 and 999 -> 1000: the header grows inside a tile; 1100 records of 20 bases fill two tiles"""
    seq = random_document(4000, 7)
    rng = np.random.default_rng(n)
    compare(engine, seq, one_column(np.full(n, 20), rng.integers(0, 3980, size=n), rng.integers(0, 2, size=n).astype(bool)), 1,
            terminators=(True,))


def test_more_records_in_a_tile_than_the_lds_table_holds(engine):
    """records of 7 or 8 bytes: more than LDS_RECORDS of them begin in one tile, whose lanes then search HBM"""
    n = 2 * TILE_BYTES // 8 + 37
    assert TILE_BYTES // 11 > LDS_RECORDS
    seq = random_document(500, 8)
    compare(engine, seq, one_column(np.zeros(n), np.zeros(n), np.ones(n, bool)), 1, dialects=(M.PYTHON,))
    compare(engine, seq, one_column(np.ones(n), np.arange(n) % 500, np.arange(n) % 3 > 0), 1, dialects=(M.BINARY,), terminators=(True,))


@pytest.mark.parametrize("plus", [True, False])
def test_one_long_record_between_short_ones(engine, plus, tmp_path):
    """about 200 kb between 20-base records: it spans many tiles and workgroups; written whole and in pieces of 4096 bytes,
    where a record begins or ends at a piece's first or last line and the long one is a piece of its own"""
    seq = random_document(260000, 9)
    lengths = np.array([20] * 7 + [200003] + [20] * 9 + [65536 + 5] + [20] * 300, np.uint32)
    rng = np.random.default_rng(10)
    starts = rng.integers(0, 50000, size=len(lengths))
    table = one_column(lengths, starts, np.full(len(lengths), plus))
    whole = compare(engine, seq, table, 1, terminators=(True,), path=str(tmp_path / "whole.fa"))
    assert whole["pieces"] >= 2                              # (the text and the file, one piece each)
    os.environ["MMT_MERGED_TEXT_PIECE"] = "4096"
    try:
        pieces = compare(engine, seq, table, 1, terminators=(True,), path=str(tmp_path / "pieces.fa"))
    finally:
        del os.environ["MMT_MERGED_TEXT_PIECE"]
    assert pieces["pieces"] > 4


def test_piece_boundaries(engine, tmp_path):
    """records of every length from 0 to 400 in pieces of 4096 bytes: pieces begin and end at every alignment"""
    seq = random_document(6000, 11)
    lengths = np.arange(401, dtype=np.uint32).repeat(2)
    rng = np.random.default_rng(12)
    table = one_column(lengths, rng.integers(0, 5500, size=len(lengths)), rng.integers(0, 2, size=len(lengths)).astype(bool))
    os.environ["MMT_MERGED_TEXT_PIECE"] = "4096"
    try:
        stats = compare(engine, seq, table, 1, path=str(tmp_path / "pieces.fa"))
    finally:
        del os.environ["MMT_MERGED_TEXT_PIECE"]
    assert stats["pieces"] > 30


def edge_rows(n):
    """starts at 0 and at the last base, around a packed word's edge and around the exception-block edge, each with lengths
    around one and two chunks, on both strands"""
    starts, lengths = [], []
    for s in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, n - 1, n - 16, n - 17, n - 33):
        for length in (1, 2, 15, 16, 17, 31, 32, 33, 48, 100):
            if 0 <= s < n:
                starts.append(s)
                lengths.append(length)
    starts, lengths = np.array(starts * 2), np.array(lengths * 2, np.uint32)
    return lengths, starts, np.arange(len(starts)) < len(starts) // 2


def test_start_positions(engine):
    seq = random_document(8200, 13)
    compare(engine, seq, one_column(*edge_rows(len(seq))), 1)
    seq = random_document(4097, 14)                         # the last base is the first of an exception block
    compare(engine, seq, one_column(*edge_rows(len(seq))), 1, terminators=(True,))


# ---- 7, 8. the engine's own text ----------------------------------------------------------------------------------------------------
def resident_documents():
    """six documents that share an ancestor with a run of N and one IUPAC byte, so that multi-MUMs hold exceptions: the runs
    differ in length from document to document (a MUM then ends or begins inside the longer ones); document 2 is the reverse
    complement, so its rows lie on '-'; document 4 is lower case"""
    rng = np.random.default_rng(21)
    anc = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=24000).astype(np.uint8)
    docs = []
    for d in range(6):
        s = anc.copy()
        for p in rng.integers(0, len(s), size=40):
            s[p] = rng.choice(np.frombuffer(b"ACGT", np.uint8))
        s[5000:5040] = ord("N")                              # wholly inside a MUM of every document
        s[9000] = ord("R")
        s[4090:4100] = ord("N")                              # across an exception-block edge
        head = s[:15000].tobytes()
        tail = s[15000:].tobytes()
        rec = head + b"N" * (30 + 3 * d) + bytes([b"ACGT"[d % 4]]) + tail      # a run that is longer from document to document
        if d == 2:
            rec = M.reverse_complement(rec)
        if d == 4:
            rec = rec.lower()
        docs.append(rec)
    return docs


def resident_child(packed):
    """runs in a process of its own: a small run, then Engine.mum_sequences and hand-made rows for every column against the
    model fed the same documents.  The engine's own rows are only counted for exceptions at their ends and inside them; that a
    run of exceptions begins, ends and lies wholly inside a range, on each strand and in each layout, is held by the hand-made
    rows.  Then the refusals only a resident source has: a table of another width than the engine's text, and a text that the
    engine has laid out again since the records were measured."""
    import tempfile
    import mumemto_amd
    docs = resident_documents()
    eng = mumemto_amd.Engine(0)
    eng.set_docs([[d] for d in docs])
    eng.run()
    assert eng.text_packed() is bool(packed), "the engine's text is not in the layout this test is about"
    lengths, starts, strands = eng.rows_mum()
    assert len(lengths) > 50 and strands[:, 0].all() and (~strands[:, 2]).sum() > 20
    upper = [d.upper() for d in docs]                        # the resident text is upper case
    held = {"begin": 0, "end": 0, "inside": 0}
    for c in range(6):
        for dialect in DIALECTS:
            want = M.sequences(upper[c], lengths, starts, strands, c, dialect)
            got = eng.mum_sequences(c, dialect)
            assert got == want, (c, dialect, first_difference(got, want))
        if c in (2, 5):                                      # where the exceptions lie in the MUMs of a '-' and a '+' column
            for length, s in zip(lengths.tolist(), starts[:, c].tolist()):
                cut = upper[c][s:s + length]
                held["begin"] += cut.startswith(b"N")
                held["end"] += cut.endswith(b"N")
                held["inside"] += b"N" in cut.strip(b"N") or b"R" in cut or b"Y" in cut
    assert held["inside"] >= 2 and held["begin"] + held["end"] >= 1, held
    first = M.sequences(upper[0], lengths, starts, strands, 0, M.PYTHON)
    assert all(eng.mum_sequences(c) == first for c in (1, 2, 3, 5))          # a multi-MUM spells the same bases in every document
    # rows of our own over the resident text: every edge, and ranges that begin, end and lie inside the runs of N
    for c in range(6):
        n = len(docs[c])
        el, es, ep = edge_rows(n)
        runs = [(a, b) for a, b in ((5000, 5040), (4090, 4100), (15000, 15030 + 3 * c))]
        if c == 2:
            runs = [(n - b, n - a) for a, b in runs]
        rl, rs = [], []
        for a, b in runs:
            for s, e in ((a - 20, a + 5), (b - 5, b + 20), (a - 40, b + 40), (a, b), (a + 1, b - 1), (a - 1, b + 1)):
                rs.append(s)
                rl.append(e - s)
        lengths_c = np.concatenate([el, np.array(rl * 2, np.uint32)])
        starts_c = np.concatenate([es, np.array(rs * 2)])
        plus_c = np.concatenate([ep, np.arange(2 * len(rs)) < len(rs)])
        tab = one_column(lengths_c, starts_c, plus_c, n_docs=6, col=c)
        with mumemto_amd.Merged.from_rows(eng, *tab) as t:
            for dialect in DIALECTS:
                want = M.sequences(upper[c], *tab, c, dialect)
                assert t.sequences(c, None, dialect) == len(want)
                got = t.sequences_text()
                assert got == want, (c, dialect, first_difference(got, want))
    with tempfile.TemporaryDirectory() as work:
        out = os.path.join(work, "refused.fa")

        def nothing_attached(m):
            for call in (m.sequences_text, lambda: m.write_sequences(out), m.sequences_offsets, m.sequences_offsets_device):
                with pytest.raises(mumemto_amd.MumemtoError) as ex:
                    call()
                assert "no sequences attached: call mmt_merged_sequences first" in str(ex.value)
            assert os.listdir(work) == []

        for width in (2, 5, 7):                              # a table of another width than the text has documents
            tab = one_column([20, 30], [100, 200], [True, False], n_docs=width, col=1)
            with mumemto_amd.Merged.from_rows(eng, *tab) as m:
                assert m.sequences(1, upper[1]) > 0          # (attached: the refusal drops it again)
                for dialect in DIALECTS:
                    with pytest.raises(mumemto_amd.MumemtoError) as ex:
                        m.sequences(1, None, dialect)
                    assert "sequences: the table has %d columns, the engine's text 6 documents" % width in str(ex.value)
                    nothing_attached(m)
        tab = one_column([20, 30], [100, 200], [True, False], n_docs=6, col=1)
        with mumemto_amd.Merged.from_rows(eng, *tab) as m:
            want = M.sequences(upper[1], *tab, 1)
            assert m.sequences(1, None) == len(want) and m.sequences_text() == want
            eng.run()                                        # the same documents, the same length: a text laid out again
            for call in (m.sequences_text, lambda: m.write_sequences(out)):
                with pytest.raises(mumemto_amd.MumemtoError) as ex:
                    call()
                assert "the engine's text is no longer the one the records were measured on" in str(ex.value)
            assert os.listdir(work) == []
            assert m.sequences(1, None) == len(want) and m.sequences_text() == want      # measured anew
            m.write_sequences(out)
            assert read(out) == want and os.listdir(work) == ["refused.fa"]
    eng.close()
    print("resident ok", held)


@pytest.mark.parametrize("packed", [0, 1], ids=["bytes", "packed"])
def test_resident_text(packed):
    env = dict(CHILD_ENV)
    env.pop("MMT_PACKED_TEXT", None)
    if packed:
        env["MMT_PACKED_TEXT"] = "1"
    r = subprocess.run([sys.executable, "-c", "import test_gpu_sequences as t; t.resident_child(%d)" % packed], cwd=ROOT,
                       capture_output=True, timeout=300, env=env)
    assert r.returncode == 0 and b"resident ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- 9 - 13 ----------------------------------------------------------------------------------------------------------------------------
SEQ = b"ACGTacgtNNRYKMSWBDHVXnAAACCCGGGTTTacgtAC"
EDGE = [(9, 36, True), (9, 36, False), (5, 40, True), (5, 40, False), (0, 3, True)]           # clipped, at the end, no bases
LENIENT = [(5, 41, True), (5, 10 ** 12, False), (5, -1, False), (70000, -1, True)]            # beyond the end, partial


def test_both_dialects_on_the_rows_they_differ_in(engine):
    import mumemto_amd
    rows = EDGE + LENIENT
    table = one_column([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], n_docs=2)
    stats = compare(engine, SEQ, table, 1, dialects=(M.PYTHON,))
    assert (stats["clipped"], stats["empty"]) == (4, 7)
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        m.sequences(1, SEQ, "python")
        assert m.sequences_text() == b">mum_0\nGTAC#\n>mum_1\nGTAC#\n" + b"\n".join(b">mum_%d\n#" % i for i in range(2, 9))
    edge = one_column([r[0] for r in EDGE], [r[1] for r in EDGE], [r[2] for r in EDGE], n_docs=2)
    compare(engine, SEQ, edge, 1, dialects=(M.BINARY,))
    with mumemto_amd.Merged.from_rows(engine, *edge) as m:
        m.sequences(1, SEQ, "binary")
        assert m.sequences_text() == b">mum_0\ngtAC#\n>mum_1\ngtAC#\n>mum_2\n#\n>mum_3\n#\n>mum_4\n#\n"


def test_refusals(engine, tmp_path):
    """every refusal: its message, nothing attached afterwards, and no file or .tmp left behind (a table of 2^32 rows does not
    fit a test: that refusal is read in sequences.cpp alone)"""
    import mumemto_amd
    L = engine.L
    out = str(tmp_path / "refused.fa")
    rows = EDGE + LENIENT
    table = one_column([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], n_docs=2)

    def refused(m, message, *args, **kw):
        with pytest.raises(mumemto_amd.MumemtoError) as ex:
            m.sequences(*args, **kw)
        assert message in str(ex.value), str(ex.value)
        for call in (m.sequences_text, lambda: m.write_sequences(out), m.sequences_offsets, m.sequences_offsets_device):
            with pytest.raises(mumemto_amd.MumemtoError) as ex:
                call()
            assert "no sequences attached: call mmt_merged_sequences first" in str(ex.value)
        assert os.listdir(str(tmp_path)) == []

    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        with pytest.raises(mumemto_amd.MumemtoError):
            m.sequences(1, SEQ, "perl")
        m.sequences(1, SEQ, "python")                        # (attached: every refusal below drops it again)
        refused(m, "sequences: column 2 is out of range (0-1)", 2, SEQ)
        refused(m, "sequences: column -1 is out of range (0-1)", -1, SEQ)
        refused(m, "sequences: row 7 has no start in column 1 (a partial multi-MUM)", 1, SEQ, "binary")
        refused(m, "sequences: row 0 has no start in column 0 (a partial multi-MUM)", 0, SEQ, "binary")
        refused(m, "sequences: the engine holds no text", 1, None)
    beyond = one_column([5, 5, 5], [3, 41, 10 ** 12], [True] * 3, n_docs=2)
    with mumemto_amd.Merged.from_rows(engine, *beyond) as m:
        refused(m, "sequences: the start 41 of row 1, column 1 lies beyond the document's end (40 bases)", 1, SEQ, "binary")
    for dialect in DIALECTS:
        below = one_column([5, 5, 5], [3, -2, -7], [True] * 3, n_docs=2)
        with mumemto_amd.Merged.from_rows(engine, *below) as m:
            refused(m, "sequences: the start -2 of row 1, column 1 lies below -1", 1, SEQ, dialect)
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        # through the ABI: a null table, null bases, an unknown dialect, a file that is not there
        k = C.c_uint64()
        assert L.mmt_merged_sequences(engine.h, None, 0, 1, 1, C.byref(k)) != 0
        assert b"must be non-null" in L.mmt_last_error()
        assert L.mmt_merged_sequences_host(engine.h, m.h, None, 40, 1, 1, 1, C.byref(k)) == 3
        assert b"sequences: null bases for a document of 40 bases" in L.mmt_last_error()
        assert L.mmt_merged_sequences_host(engine.h, m.h, SEQ, 40, 1, 2, 1, C.byref(k)) == 3
        assert b"sequences: unknown dialect 2" in L.mmt_last_error()
        assert L.mmt_merged_sequences_file(engine.h, m.h, os.fsencode(str(tmp_path / "gone.fa")), 1, 1, 1, None, C.byref(k)) == 3
        assert L.mmt_merged_sequences_text(None, None) is None and L.mmt_merged_sequences_write_text(m.h, None) != 0
        assert os.listdir(str(tmp_path)) == []
        st = (C.c_double * 8)()
        assert L.mmt_merged_sequences_stats(m.h, st) == 0 and list(st)[2:7] == [0.0] * 5


def test_merge_driver_reports_partial_mums_and_cleans_up(tmp_path, monkeypatch):
    from mumemto_amd import merge_mums, mumsio
    monkeypatch.setenv("MUMEMTO_NO_TORCH", "1")
    seq = random_document(3000, 15, plain=True)
    for name in ("a", "b"):
        with open(str(tmp_path / (name + ".fa")), "wb") as f:
            f.write(b">x\n" + seq + b"\n")
        (tmp_path / (name + ".lengths")).write_text("%s 3000\n%s 3000\n" % (tmp_path / (name + ".fa"), tmp_path / (name + ".fa")))
        (tmp_path / (name + ".thresh")).write_bytes(b"")
        (tmp_path / (name + ".thresh_rev")).write_bytes(b"")
    mumsio.write_mums(str(tmp_path / "a.mums"), np.array([30, 40], np.uint32), np.array([[5, 900], [100, 2000]]), np.ones((2, 2), bool))
    args = merge_mums.parse_arguments([str(tmp_path / "a.mums"), str(tmp_path / "b.mums"), "-o", str(tmp_path / "out"),
                                       "--extract-on-device"])
    # no start in the first document, and none in a later one: the binary stops at either, and so does this path
    for partial in ("30\t5,900\t+,+\n40\t,2000\t+,+\n", "30\t5,900\t+,+\n40\t100,\t+,+\n"):
        (tmp_path / "b.mums").write_text(partial)
        with pytest.raises(SystemExit) as ex:
            merge_mums.run_merger(args)
        assert ex.value.code == 1
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(("_mums.fa", ".tmp"))]


def test_empty_table_gives_an_empty_text(engine, tmp_path):
    import mumemto_amd
    table = (np.zeros(0, np.uint32), np.zeros((0, 3), np.int64), np.zeros((0, 3), bool))
    out = str(tmp_path / "empty.fa")
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        for dialect in DIALECTS:
            assert m.sequences(2, SEQ, dialect) == 0 and m.sequences_text() == b""
            m.write_sequences(out)
            assert read(out) == b"" and os.listdir(str(tmp_path)) == ["empty.fa"]
            assert m.sequences_offsets().tolist() == [0]
    assert M.sequences(SEQ, *table, 2) == b""


def test_the_last_column_of_a_table(engine):
    seq = random_document(5000, 16)
    rng = np.random.default_rng(17)
    n = 333
    compare(engine, seq, one_column(rng.integers(0, 90, size=n), rng.integers(0, 4950, size=n), rng.integers(0, 2, size=n).astype(bool),
                                    n_docs=94, col=93), 93, terminators=(True,))


def test_housekeeping(engine):
    """the ABI version stays; sequences() only reads: rows, blocks and BED records are what they were"""
    import mumemto_amd
    assert engine.L.mmt_abi_version() == 7
    rng = np.random.default_rng(18)
    n = 400
    lengths = rng.integers(20, 200, size=n).astype(np.uint32)
    starts = np.sort(rng.integers(0, 90000, size=n))[:, None] + np.array([0, 500, 1000])
    strands = np.ones((n, 3), bool)
    seq = random_document(100000, 19)
    contigs = ([["c0"], ["c1"], ["c2"]], [[200000], [200000], [200000]])
    with mumemto_amd.Merged.from_rows(engine, lengths, starts, strands) as m:
        blocks = m.collinear(1000, None)
        m.bed(contigs, None, 0)
        before = [a.copy() for a in m.rows()] + [m.blocks().copy()] + [a.copy() for a in m.bed_records()] + [m.bed_text(1)]
        for dialect in DIALECTS:
            got_len = m.sequences(2, seq, dialect)
            rows = m.rows()
            assert m.sequences_text() == M.sequences(seq, rows[0], rows[1], rows[2], 2, dialect) and got_len > 0
        after = list(m.rows()) + [m.blocks()] + list(m.bed_records()) + [m.bed_text(1)]
        assert len(blocks) == len(after[3]) and all(np.array_equal(a, b) for a, b in zip(before, after))
        assert m.sequences_offsets_device() != 0
        m.collinear(1000, None)                              # a new table drops the sequences
        with pytest.raises(mumemto_amd.MumemtoError):
            m.sequences_text()
