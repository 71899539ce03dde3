"""GPU: the BED writer (csrc/bed.cpp, bed_kernels.hip) against the files the reference's own tool wrote (tests/golden/bed) and
against the closed-form host model tests/bedmodel.py, which tests/test_bed_host.py holds to the same files and to a plain
loop.  Every comparison is exact: record offsets, records and text bytes."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bedmodel as M
import collmodel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "bed")
BEDS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "*.bed")))
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1")       # (the tool needs no tensor library: a quicker start)
TOOL = [sys.executable, "-m", "mumemto_amd.mum_to_bed"]


def kernel_constant(name):
    text = open(os.path.join(ROOT, "mumemto_amd", "csrc", "bed_kernels.hpp")).read()
    return int(re.search(r"%s\s*=\s*(\d+)" % name, text).group(1))


TILE = kernel_constant("SELECT_BLOCK") * kernel_constant("SELECT_ITEMS")     # rows of one workgroup of the select
WAVE = kernel_constant("BED_WAVE_RECORDS")                                   # records of one wave of the writer
LDS_CONTIGS = kernel_constant("BED_LDS_CONTIGS")                             # contig ends a workgroup of the lookup stages
LDS_BYTES = kernel_constant("BED_LDS_BYTES")                                 # the longest span of lines a wave stages
assert (TILE, WAVE, LDS_CONTIGS, LDS_BYTES) == (1024, 64, 1024, 8192)


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def device(engine, table, contigs, seq_idx=None, L=100, blocks=None):
    import mumemto_amd
    with mumemto_amd.Merged.from_rows(engine, *table[:3]) as m:
        if blocks is not None:
            m.set_blocks(blocks)
        k = m.bed(contigs, seq_idx, L)
        record_begin, records = m.bed_records()
        assert k == len(records)
        cols = range(m.n_docs) if seq_idx is None else [seq_idx]
        texts = {c: m.bed_text(c) for c in cols}
        return record_begin, records, texts, m.bed_stats()


def check(engine, table, contigs, seq_idx=None, L=100, blocks=None, tag=""):
    want = M.bed(table[0], table[1], table[2], contigs, seq_idx, L, blocks)
    got = device(engine, table, contigs, seq_idx, L, blocks)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]), (tag, got[0][:8], want[0][:8])
    assert got[1].shape == want[1].shape, (tag, got[1].shape, want[1].shape)
    bad = np.nonzero((got[1] != want[1]).any(axis=1))[0]
    assert not len(bad), (tag, bad[:4], got[1][bad[:4]], want[1][bad[:4]])
    total = 0
    for c, text in got[2].items():
        lines = M.text(want[1][int(want[0][c]):int(want[0][c + 1])], contigs[0][c])
        assert text == lines, (tag, c, text[:200], lines[:200])
        total += len(lines)
    stats = got[3]
    assert (stats["records"], stats["clamped"], stats["text_bytes"]) == (len(want[1]), want[2], total), (tag, stats)
    return want, stats


def rows_with_contigs(seed, n, n_docs, counts=None, absent=0.0, base=0, **kw):
    t = M.make_rows(seed, n, n_docs, absent=absent, base=base)
    return t, M.make_contigs(seed + 1000, t[3], counts or [1 + 3 * c for c in range(n_docs)], **kw)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------
def recorded(bed):
    m = re.fullmatch(r"(\w+?)((?:\.g\d+)?)\.s(\d+)\.L(\d+)\.bed", bed)
    return (os.path.join(GOLD, m.group(1) + m.group(2) + ".mums"), os.path.join(GOLD, m.group(1) + ".lengths"), int(m.group(3)),
            int(m.group(4)))


def table_of(path):
    from mumemto_amd import mumsio
    from mumemto_amd.find_inversions import blocks_of_rows
    lengths, starts, strands, row_block = mumsio.read_mums(path, with_blocks=True)
    return lengths, starts, strands, None if row_block is None else blocks_of_rows(row_block)


def expected_of(bed):
    """the recorded bytes; for a table that ends in a block, with the line the reference never flushes (departure 1)"""
    from mumemto_amd import mumsio
    path, lens_path, s, L = recorded(bed)
    t = table_of(path)
    want = open(os.path.join(GOLD, bed), "rb").read()
    if M.ends_in_block(t[3], len(t[0])):
        contigs = mumsio.read_contigs(lens_path)
        assert M.bed_bytes(*t[:3], s, contigs, L, t[3], drop_open_tail=True) == want
        want = M.bed_bytes(*t[:3], s, contigs, L, t[3])
    return want


@pytest.mark.parametrize("bed", BEDS, ids=[b[:-4] for b in BEDS])
def test_golden_through_the_abi(engine, bed):
    from mumemto_amd import mumsio
    path, lens_path, s, L = recorded(bed)
    t = table_of(path)
    contigs = mumsio.read_contigs(lens_path)
    got = device(engine, t, contigs, s, L, t[3])
    assert got[2][s] == expected_of(bed)
    check(engine, t, contigs, s, L, t[3], bed)


@pytest.mark.parametrize("bed", ["synteny.g1000.s0.L100", "inversion.g1000.s3.L0", "moved.g1000.s3.L100", "moved.g0.s1.L0",
                                 "minus_column.g1000.s2.L0", "minus_column.g0.s3.L100", "partial.s1.L0", "partial.s4.L100"])
def test_golden_through_the_tool(bed, tmp_path):
    """`python -m mumemto_amd.mum_to_bed` as a fresh child process: the reference's flags, the reference's bytes in the file
    the library wrote (plus the last block's line where the table ends in one)"""
    path, lens_path, s, L = recorded(bed + ".bed")
    out = str(tmp_path / "out.bed")
    r = subprocess.run(TOOL + [path, "-l", lens_path, "-s", str(s), "-L", str(L), "-o", out], cwd=ROOT, capture_output=True,
                       timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b"", r.stderr.decode()
    assert open(out, "rb").read() == expected_of(bed + ".bed")
    assert not os.path.exists(out + ".tmp")


def test_tool_stdout_verbose_all_and_gap(tmp_path):
    want = expected_of("inversion.g1000.s7.L100.bed")
    base = [os.path.join(GOLD, "inversion.g1000.mums"), "-l", os.path.join(GOLD, "inversion.lengths"), "-s", "7"]
    r = subprocess.run(TOOL + base, cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == want and r.stderr == b"", r.stderr.decode()
    r = subprocess.run(TOOL + base + ["-v"], cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == want and b"12 blocks" in r.stderr          # -v never changes the output
    # the table without the block field and -g 1000: the blocks the reference's collinear tool wrote into the other file
    r = subprocess.run(TOOL + [os.path.join(GOLD, "inversion.mums"), "-g", "1000"] + base[1:], cwd=ROOT, capture_output=True,
                       timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()
    prefix = str(tmp_path / "all")
    r = subprocess.run(TOOL + [base[0], "-l", base[2], "--all", "-L", "0", "-o", prefix], cwd=ROOT, capture_output=True, timeout=120,
                       env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert sorted(os.listdir(str(tmp_path))) == ["all.%d.bed" % c for c in range(8)]
    for c in (0, 1, 3, 7):
        assert open("%s.%d.bed" % (prefix, c), "rb").read() == expected_of("inversion.g1000.s%d.L0.bed" % c), c


# ---- sizes -------------------------------------------------------------------------------------------------------------
# the edges of a wave of the writer (64 records, so that a staged span ends inside and across a line), of a tile of the select
# and of two tiles; without blocks and with -L 0 every row is a record
@pytest.mark.parametrize("n", [0, 1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_counts(engine, n):
    t, contigs = rows_with_contigs(n, n, 3)
    want, stats = check(engine, t, contigs, None, 0, tag=n)
    assert len(want[1]) == 3 * n and stats["batches"] == (3 if n else 0)
    blocks = M.make_blocks(n, n)
    want, stats = check(engine, t, contigs, None, 100, blocks, tag=(n, "blocks"))
    assert stats["batches"] == (1 if len(want[1]) else 0)
    if n >= WAVE:
        assert (want[1][:, 3] >= 0).any() and (want[1][:, 3] < 0).any()


@pytest.mark.parametrize("k", [WAVE - 1, WAVE, WAVE + 1, 4 * WAVE + 1])
@pytest.mark.parametrize("name_len", [1, 200])
def test_record_counts_and_name_lengths(engine, k, name_len):
    """names of 1 byte: the lines of a wave are staged in LDS; of 200: their span is longer than the stage and they go out on
    their own; one-row blocks and rows alternate"""
    t = M.make_rows(7, k, 2)
    contigs = M.make_contigs(8, t[3], [3, 9], name_len=(name_len, name_len + 1))
    contigs = ([[("n" * name_len if name_len == 200 else "cdefghijklmn"[j % 12]) for j in range(len(seq))] for seq in contigs[0]],
               contigs[1])
    assert (WAVE - 1) * (name_len + 20) > LDS_BYTES if name_len == 200 else WAVE * (name_len + 60) <= LDS_BYTES
    blocks = np.array([(r, r) for r in range(0, k, 2)], np.uint32)
    want, _ = check(engine, t, contigs, None, 0, blocks, tag=(k, name_len))
    assert len(want[1]) == 2 * k


# ---- shapes of blocks --------------------------------------------------------------------------------------------------
def test_blocks_across_tile_boundaries_at_both_ends_and_on_minus(engine):
    n = 2 * TILE + 1
    t, contigs = rows_with_contigs(21, n, 4)
    t[2][:, 1] = False                                       # a column on '-' throughout
    blocks = np.array([(0, 5), (TILE - 3, TILE + 2), (TILE + 3, TILE + 3), (2 * TILE - 1, 2 * TILE)], np.uint32)
    want, _ = check(engine, t, contigs, None, 100, blocks)
    col1 = want[1][int(want[0][1]):int(want[0][2])]
    assert (col1[:, 4] == 0).all() and (col1[:, 3] >= 0).sum() == 4
    assert col1[0][3] == 0 and col1[-1][3] == 3              # the table begins and ends in a block
    check(engine, t, contigs, 1, 0, blocks)


def test_one_block_every_row_a_block_and_nothing_selected(engine):
    n = TILE + 77
    t, contigs = rows_with_contigs(22, n, 3)
    want, _ = check(engine, t, contigs, None, 100, np.array([(0, n - 1)], np.uint32))
    assert len(want[1]) == 3
    want, _ = check(engine, t, contigs, None, 100, np.array([(r, r) for r in range(n)], np.uint32))
    assert len(want[1]) == 3 * n and (want[1][:, 3] >= 0).all()
    for blocks in (None, np.zeros((0, 2), np.uint32)):
        want, stats = check(engine, t, contigs, None, 1 << 40, blocks)
        assert len(want[1]) == 0 and stats["text_bytes"] == 0
    check(engine, t, contigs, 2, 0, np.zeros((0, 2), np.uint32))               # blocks attached, none there: every row


def test_partial_rows_without_blocks_number_by_rank(engine):
    t, contigs = rows_with_contigs(23, TILE + 300, 5, absent=0.35)
    want, _ = check(engine, t, contigs, None, 0)
    for c in range(5):
        rec = want[1][int(want[0][c]):int(want[0][c + 1])]
        assert (-1 - rec[:, 3]).tolist() == list(range(len(rec))) and len(rec) == (t[1][:, c] != -1).sum() < len(t[0])
    want, _ = check(engine, t, contigs, None, 200)
    rec = want[1][int(want[0][3]):int(want[0][4])]
    assert not np.array_equal(-1 - rec[:, 3], np.arange(len(rec)))
    check(engine, t, contigs, 4, 150)


# ---- columns and contigs -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """94 columns; column 5 has as many contigs as the lookup stages in LDS, column 6 one more: both routes run"""
    t = M.make_rows(31, 700, 94)
    counts = [1 + (7 * c) % 50 for c in range(94)]
    counts[5], counts[6] = LDS_CONTIGS, LDS_CONTIGS + 1
    contigs = M.make_contigs(32, t[3], counts, zero=0.1)
    blocks = M.make_blocks(33, 700)
    return t, contigs, blocks, M.bed(t[0], t[1], t[2], contigs, None, 100, blocks)


def test_94_columns_and_both_lookup_routes(engine, wide):
    t, contigs, blocks, want = wide
    got, stats = check(engine, t, contigs, None, 100, blocks)
    for c in (5, 6):
        assert len(set(want[1][int(want[0][c]):int(want[0][c + 1]), 0].tolist())) > 100       # many contigs are hit
    assert stats["batches"] == 1


@pytest.mark.parametrize("batch", ["1", "7", "1000"])
def test_column_batches(engine, wide, batch):
    t, contigs, blocks, want = wide
    os.environ["MMT_COLLINEAR_BATCH"] = batch
    try:
        got = device(engine, t, contigs, None, 100, blocks)
    finally:
        del os.environ["MMT_COLLINEAR_BATCH"]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[3]["batches"] == {"1": 94, "7": 14, "1000": 1}[batch]


def test_single_columns_equal_the_pass_over_all(engine, wide):
    import mumemto_amd
    t, contigs, blocks, want = wide
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        m.set_blocks(blocks)
        for c in (0, 5, 6, 50, 93):
            m.bed(contigs, c, 100)
            record_begin, records = m.bed_records()
            assert record_begin[c] == 0 and (record_begin[c + 1:] == len(records)).all(), c
            assert np.array_equal(records, want[1][int(want[0][c]):int(want[0][c + 1])]), c


def test_one_contig_empty_contigs_boundaries_and_the_clamp(engine):
    lengths = np.array([50, 60, 70, 80], np.uint32)
    starts = np.array([[0, 10], [100, 99], [200, 250], [300, 400]], np.int64)
    table = (lengths, starts, np.array([[True, False]] * 4))
    # column 0: boundaries exactly on the starts 100 and 200, empty contigs around them; column 1: one contig
    contigs = ([["e0", "a", "e1", "e2", "b", "c", "e3"], ["only"]], [[0, 100, 0, 0, 100, 1000, 0], [10**6]])
    want, stats = check(engine, table, contigs, None, 0)
    assert want[1][:4].tolist() == [[1, 0, 50, -1, 1], [4, 0, 60, -2, 1], [5, 0, 70, -3, 1], [5, 100, 180, -4, 1]]
    assert (want[1][4:, 0] == 0).all() and stats["clamped"] == 0
    # the sequences end early: starts at (300 == total) and beyond (400 > 260) the end get the last contig and are counted
    contigs = ([["a", "b", "e"], ["p", "q"]], [[100, 200, 0], [250, 10]])
    want, stats = check(engine, table, contigs, None, 0)
    assert want[1][3].tolist() == [2, 0, 80, -4, 1] and want[1][7].tolist() == [1, 150, 230, -4, 0] and stats["clamped"] == 2
    assert check(engine, table, contigs, 1, 0)[1]["clamped"] == 1


def test_values_of_1_to_13_digits(engine):
    base = (1 << 40) + 3
    t = M.make_rows(41, 500, 2, base=base)
    t[1][:, 0] -= base                                      # column 0 from 0 upwards, column 1 beyond 2^40
    assert t[1][0, 0] == 0 and t[1][:, 1].min() > 1 << 40
    cut = int(t[1][1, 1])                                    # a boundary on the second start: 13 digits before it, 1 behind
    contigs = ([["chr1", "chr2"], ["u", "v", "w"]], [[t[3][0] - base - 10, 10], [cut, 7, t[3][1] - cut - 7]])
    want, _ = check(engine, t, contigs, None, 0)
    digits = {len(str(v)) for v in want[1][:, 1].tolist()}
    assert {1, 13} <= digits and len(digits) >= 5


# ---- the table and what hangs on it ------------------------------------------------------------------------------------
def test_refusals(engine):
    import ctypes as C
    import mumemto_amd
    t, contigs = rows_with_contigs(51, 50, 3)
    empty = [0] * len(contigs[1][1])
    negative = list(contigs[1][2])
    negative[1] = -1
    bad = lambda names=None, lens=None: (names or contigs[0], lens or contigs[1])      # noqa: E731
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        assert engine.L.mmt_merged_bed_records(m.h, None, None) == 3 and b"no BED records" in engine.L.mmt_last_error()
        with pytest.raises(mumemto_amd.MumemtoError, match="no BED records attached"):
            m.bed_text(0)
        for idx, c, msg in ((3, contigs, "out of range"), (-2, contigs, "out of range"),
                            (1, bad(lens=[contigs[1][0], empty, contigs[1][2]]), "total length 0"),
                            (None, bad(lens=[contigs[1][0], contigs[1][1], negative]), "negative length"),
                            (None, bad([contigs[0][0], [], contigs[0][2]], [contigs[1][0], [], contigs[1][2]]), "no contigs")):
            with pytest.raises(mumemto_amd.MumemtoError, match=msg):
                m.bed(c, idx)
        assert engine.L.mmt_merged_bed(engine.h, m.h, None, None, None, None, 0, 100, None) == 3
        assert b"contig_begin" in engine.L.mmt_last_error()
        begin, lens, name_begin, blob = mumemto_amd.binding.contig_tables(contigs)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert engine.L.mmt_merged_bed(engine.h, m.h, p(begin), None, p(name_begin), blob, 0, 100, None) == 3
        tabbed = np.frombuffer(blob.replace(b"s1c0", b"s\tc0", 1), np.uint8)
        assert engine.L.mmt_merged_bed(engine.h, m.h, p(begin), p(lens), p(name_begin), p(tabbed), 1, 100, None) == 3
        assert b"tab or a newline" in engine.L.mmt_last_error()
        assert engine.L.mmt_merged_bed(engine.h, m.h, p(begin), p(lens), p(name_begin), p(tabbed), 0, 100, None) == 0   # not needed
        m.bed(bad(lens=[contigs[1][0], empty, contigs[1][2]]), 0)                  # a column that is not needed is not looked at
        with pytest.raises(mumemto_amd.MumemtoError, match="out of range"):
            m.bed_text(3)
        assert engine.L.mmt_merged_bed_write_text(m.h, -1, b"/dev/null") == 3


def test_a_column_written_in_pieces_is_the_column_written_whole(engine, tmp_path):
    """bed_write_text cuts a column into pieces of whole lines (MMT_MERGED_TEXT_PIECE is the test hook; 256 MB otherwise): two
    columns of 402 records, in column 1 a contig whose name alone is longer than a piece, so that its lines are pieces of
    their own; the files equal bed_text with the hook and without it"""
    import mumemto_amd
    t = M.make_rows(77, 1400, 2)
    blocks = M.make_blocks(78, 1400)
    names, lens = M.make_contigs(79, t[3], [3, 40])
    want = M.bed(t[0], t[1], t[2], (names, lens), None, 100, blocks)
    assert want[0].tolist() == [0, 402, 804]
    middle = int(want[1][402 + 201][0])                       # the contig of a record in the middle of column 1
    names = [list(names[0]), list(names[1])]
    names[1][middle] = "contig_" + "n" * 5000
    contigs = (names, lens)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        m.set_blocks(blocks)
        assert m.bed(contigs) == 804
        whole = [m.bed_text(c) for c in range(2)]
        for c in range(2):
            assert whole[c] == M.text(want[1][402 * c:402 * (c + 1)], names[c])
            assert len(whole[c]) > 2 * 4096                   # more than one piece of 4096 bytes
        long_lines = [l for l in whole[1].split(b"\n") if len(l) > 4096]
        assert 0 < len(long_lines) < 10 and not [l for l in whole[0].split(b"\n") if len(l) > 4096]
        for piece in (4096, None):
            for c in range(2):
                path = str(tmp_path / ("c%d.%s.bed" % (c, piece)))
                if piece:
                    os.environ["MMT_MERGED_TEXT_PIECE"] = str(piece)
                try:
                    m.write_bed(c, path)
                finally:
                    os.environ.pop("MMT_MERGED_TEXT_PIECE", None)
                assert open(path, "rb").read() == whole[c], (piece, c)
                assert not os.path.exists(path + ".tmp")


def test_results_are_dropped_with_the_blocks_and_the_table(engine):
    import mumemto_amd
    t = collmodel.make_table(93, 300, 4, inversions=[(2, 40, 200)])
    with mumemto_amd.Merged.from_rows(engine, *t) as m:
        blk = m.collinear(1000)
        calls = m.inversions()
        rows = [a.copy() for a in m.rows()]
        totals = (rows[1].max(axis=0) + 500).tolist()
        contigs = M.make_contigs(61, totals, [1, 4, 9, 30])
        covered = m.coverage(totals)
        runs = m.coverage_runs()
        assert len(blk) and len(calls)
        want = M.bed(rows[0], rows[1], rows[2], contigs, None, 100, blk)
        assert m.bed(contigs) == len(want[1]) > 0
        got = m.bed_records()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # a pure reader: rows, blocks, calls and coverage are what they were
        assert all(np.array_equal(a, b) for a, b in zip(m.rows(), rows)) and np.array_equal(m.blocks(), blk)
        out = np.zeros((len(calls), 5), np.int64)
        assert engine.L.mmt_merged_inversion_calls(m.h, out.ctypes.data) == 0 and np.array_equal(out, calls)
        again = m.coverage_runs()
        assert np.array_equal(again[0], runs[0]) and np.array_equal(again[1], runs[1]) and covered.sum() > 0
        for drop in (lambda: m.set_blocks(blk), lambda: m.collinear(1000)):
            drop()
            assert engine.L.mmt_merged_bed_records(m.h, None, None) == 3 and m.bed_stats()["records"] == 0
            with pytest.raises(mumemto_amd.MumemtoError, match="no BED records attached"):
                m.bed_records_device()
            assert m.bed(contigs) == len(want[1])


def test_sort_like_direct_drops_the_results():
    import mumemto_amd
    from mumemto_amd import synth
    docs = synth.pangenome(2, 1531, 0.02, seed=5)
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_docs(docs)
        eng.run(merge_metadata=True)
        n, nd, a, b, c = eng.rows_mum_device()
        assert n > 3 and nd == 2
        with mumemto_amd.Merged.from_device(eng, n, nd, a, b, c) as m:
            contigs = ([["x"], ["y"]], [[10000], [10000]])
            assert m.bed(contigs, None, 0) == 2 * n
            assert eng.L.mmt_merged_sort_like_direct(eng.h, m.h) == 0
            assert eng.L.mmt_merged_bed_records(m.h, None, None) == 3
            assert m.bed(contigs, None, 0) == 2 * n
    finally:
        eng.close()


def test_records_in_hbm_and_the_written_file(engine, tmp_path):
    import torch
    import mumemto_amd
    from mumemto_amd.dist import DevicePointerView
    t, contigs = rows_with_contigs(66, 3000, 4)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        m.bed(contigs, None, 0)
        record_begin, records = m.bed_records()
        a, b = m.bed_records_device()
        assert a and b and len(records) == 12000
        d_begin = torch.as_tensor(DevicePointerView(a, (5,), "<i8"), device="cuda:0").cpu().numpy()
        d_rec = torch.as_tensor(DevicePointerView(b, (len(records), 5), "<i8"), device="cuda:0").cpu().numpy()
        assert np.array_equal(d_begin.astype(np.uint64), record_begin) and np.array_equal(d_rec, records)
        out = str(tmp_path / "col2.bed")
        before = m.bed_stats()["text_bytes"]
        m.write_bed(2, out)
        want = M.text(records[int(record_begin[2]):int(record_begin[3])], contigs[0][2])
        assert open(out, "rb").read() == want and not os.path.exists(out + ".tmp")
        assert m.bed_stats()["text_bytes"] == before + len(want) and m.bed_stats()["text_ms"] > 0
        m.write_bed(2, "/dev/null")                          # a sink that is no regular file is written as it is
        assert not os.path.exists("/dev/null.tmp")
        with pytest.raises(mumemto_amd.MumemtoError, match="cannot write"):
            m.write_bed(2, str(tmp_path / "no" / "such" / "dir.bed"))


def test_python_front_door():
    import mumemto_amd
    t, contigs = rows_with_contigs(67, 400, 3)
    blocks = M.make_blocks(68, 400)
    want = M.bed(t[0], t[1], t[2], contigs, None, 100, blocks)
    got = mumemto_amd.mum_to_bed(t[0], t[1], t[2], contigs, blocks=blocks)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2] == {c: M.text(want[1][int(want[0][c]):int(want[0][c + 1])], contigs[0][c]) for c in range(3)}
    want = M.bed(t[0], t[1], t[2], contigs, 1, 0)
    got = mumemto_amd.mum_to_bed(t[0], t[1], t[2], contigs, seq_idx=1, min_singleton_length=0)
    assert np.array_equal(got[1], want[1]) and list(got[2]) == [1]
