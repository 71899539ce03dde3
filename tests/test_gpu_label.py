"""GPU: the contig labels (csrc/label.cpp, label_kernels.hip) against the files the reference's own tool wrote
(tests/golden/label) and against the host model tests/labelmodel.py, which tests/test_label_host.py holds to the same files and to
a plain loop.  Every comparison is exact: contigs, offsets and text bytes."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bedmodel
import collmodel
import labelmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "label")
LABELLED = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "*.labeled.mums")) + glob.glob(os.path.join(GOLD, "*.named.mums")))
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1")       # (the tool needs no tensor library: a quicker start)
TOOL = [sys.executable, "-m", "mumemto_amd.get_sequence_info"]


def kernel_constant(name, header="label_kernels.hpp"):
    text = open(os.path.join(ROOT, "mumemto_amd", "csrc", header)).read()
    return int(re.search(r"%s\s*=\s*(\d+)" % name, text).group(1))


TILE = kernel_constant("LABEL_ROWS")                                   # rows of one tile of the lookup
COLS = kernel_constant("LABEL_COLS")                                   # columns of one batch of the lookup
LDS_CONTIGS = kernel_constant("BED_LDS_CONTIGS", "bed_kernels.hpp")    # the staging unit: ends of one column
LDS_UNITS = kernel_constant("LABEL_LDS_UNITS")                         # units of a workgroup's pool
assert (TILE, COLS, LDS_CONTIGS, LDS_UNITS) == (64, 32, 1024, 4)


def hbm_columns(counts):
    """the rule of label.cpp: per batch of COLS columns the pool of LDS_UNITS x LDS_CONTIGS ends goes to the columns of at most
    LDS_CONTIGS contigs, fewest first, while they fit; the others are searched in HBM"""
    out = 0
    for c0 in range(0, len(counts), COLS):
        used = 0
        for k in sorted(counts[c0:c0 + COLS]):
            if k > LDS_CONTIGS or used + k > LDS_UNITS * LDS_CONTIGS:
                out += 1
            else:
                used += k
    return out


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def device(engine, table, contigs, names=False, blocks=None):
    import mumemto_amd
    with mumemto_amd.Merged.from_rows(engine, *table[:3]) as m:
        if blocks is not None:
            m.set_blocks(blocks)
        k = m.label(contigs, names)
        contig, rel = m.label_cells()
        text = m.label_text()
        assert k == len(text)
        return contig, rel, text, m.label_stats()


def check(engine, table, contigs, names=False, blocks=None, tag=""):
    want = M.label(table[0], table[1], table[2], contigs, blocks, names)
    got = device(engine, table, contigs, names, blocks)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int64
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (tag, got[0].shape, want[0].shape)
    bad = np.argwhere((got[0] != want[0]) | (got[1] != want[1]))
    assert not len(bad), (tag, bad[:4], [(got[0][r, c], got[1][r, c], want[0][r, c], want[1][r, c]) for r, c in bad[:4]])
    if got[2] != want[2]:
        a, b = got[2].split(b"\n"), want[2].split(b"\n")
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        assert False, (tag, first, len(got[2]), len(want[2]), a[first][:300], b[first][:300])
    stats = got[3]
    counts = [len(seq) for seq in contigs[1]]
    assert (stats["cells"], stats["absent"], stats["text_bytes"], stats["hbm_columns"]) == \
        (want[0].size, int((np.asarray(table[1]) == -1).sum()), len(want[2]), hbm_columns(counts)), (tag, stats)
    return want, stats


def rows_with_contigs(seed, n, n_docs, counts=None, absent=0.0, base=0, **kw):
    t = M.make_rows(seed, n, n_docs, absent=absent, base=base)
    return t, M.make_contigs(seed + 1000, t[3], counts or [1 + 3 * c for c in range(n_docs)], **kw)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------
def recorded(name):
    m = re.fullmatch(r"(\w+?)((?:\.g\d+)?)\.(labeled|named)\.mums", name)
    return os.path.join(GOLD, m.group(1) + m.group(2) + ".mums"), os.path.join(GOLD, m.group(1) + ".lengths"), m.group(3) == "named"


def table_of(path):
    from mumemto_amd import mumsio
    from mumemto_amd.find_inversions import blocks_of_rows
    lengths, starts, strands, row_block = mumsio.read_mums(path, with_blocks=True)
    return lengths, starts, strands, None if row_block is None else blocks_of_rows(row_block)


@pytest.mark.parametrize("name", LABELLED, ids=[f[:-5] for f in LABELLED])
def test_golden_through_the_abi(engine, name, tmp_path):
    import mumemto_amd
    from mumemto_amd import mumsio
    path, lens_path, named = recorded(name)
    t = table_of(path)
    contigs = mumsio.read_contigs(lens_path)
    want = open(os.path.join(GOLD, name), "rb").read()
    model = M.label(t[0], t[1], t[2], contigs, t[3], named)
    out = str(tmp_path / "out.mums")
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        if t[3] is not None:
            m.set_blocks(t[3])
        assert m.label(contigs, named) == len(want)
        contig, rel = m.label_cells()
        assert np.array_equal(contig, model[0]) and np.array_equal(rel, model[1])
        assert m.label_text() == want
        m.write_label(out)
    assert open(out, "rb").read() == want and not os.path.exists(out + ".tmp")


@pytest.mark.parametrize("name", ["synteny.g1000.labeled", "inversion.g0.named", "minus_column.g1000.labeled", "moved.g0.named",
                                  "partial.labeled", "partial.named"])
def test_golden_through_the_tool(name, tmp_path):
    """`python -m mumemto_amd.get_sequence_info` as a fresh child process: the reference's flags, the reference's bytes in the
    file the library wrote"""
    path, lens_path, named = recorded(name + ".mums")
    out = str(tmp_path / "out.mums")
    r = subprocess.run(TOOL + ["-m", path, "-l", lens_path, "-o", out] + (["-n"] if named else []), cwd=ROOT, capture_output=True,
                       timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b"", r.stderr.decode()
    assert open(out, "rb").read() == open(os.path.join(GOLD, name + ".mums"), "rb").read()
    assert not os.path.exists(out + ".tmp")


def test_tool_departures(tmp_path):
    """a start beyond the total stops the tool and names the cell; a file with `-` on every row gets `-` on every row"""
    from mumemto_amd import mumsio
    t = table_of(os.path.join(GOLD, "synteny.g1000.mums"))
    contigs = mumsio.read_contigs(os.path.join(GOLD, "synteny.lengths"))
    src, lens = str(tmp_path / "t.mums"), os.path.join(GOLD, "synteny.lengths")
    mumsio.write_mums(src, t[0], t[1], t[2], np.full(len(t[0]), mumsio.NO_BLOCK, np.uint32))
    r = subprocess.run(TOOL + ["-m", src, "-l", lens, "-v"], cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and b"0 blocks" in r.stderr, r.stderr.decode()
    want = M.label(t[0], t[1], t[2], contigs, np.zeros((0, 2), np.uint32))[2]
    assert open(str(tmp_path / "t_labeled.mums"), "rb").read() == want and want.count(b"\t-\t") == len(t[0])
    starts = t[1].copy()
    starts[7, 2] = sum(contigs[1][2])
    mumsio.write_mums(src, t[0], starts, t[2])
    out = str(tmp_path / "never.mums")
    r = subprocess.run(TOOL + ["-m", src, "-l", lens, "-o", out], cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 1 and b"row 7, column 2" in r.stderr and not os.path.exists(out), r.stderr.decode()


# ---- sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", [1, 2, 63, 64, 65, 130])
def test_column_counts(engine, n_docs):
    """one column, less than, exactly and more than a wave's worth of cells in a row, batches of the lookup that end inside one"""
    t, contigs = rows_with_contigs(n_docs, 150, n_docs, counts=[1 + (5 * c) % 23 for c in range(n_docs)], absent=0.1)
    check(engine, t, contigs, False, tag=n_docs)
    check(engine, t, contigs, True, tag=(n_docs, "names"))


@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_counts(engine, n):
    t, contigs = rows_with_contigs(n, n, 5, absent=0.2)
    want, stats = check(engine, t, contigs, False, tag=n)
    assert len(want[2]) > 0 or n == 0
    if n:                                                    # blocks want full rows
        full, contigs = rows_with_contigs(n + 500, n, 5)
        check(engine, full, contigs, True, bedmodel.make_blocks(n, n), tag=(n, "names, blocks"))


def test_no_rows_and_no_blocks_write_an_empty_file(engine, tmp_path):
    import mumemto_amd
    empty = (np.zeros(0, np.uint32), np.zeros((0, 3), np.int64), np.zeros((0, 3), bool))
    contigs = ([["a"], ["b"], ["c"]], [[5], [6], [7]])
    with mumemto_amd.Merged.from_rows(engine, *empty) as m:
        assert m.label(contigs) == 0 and m.label_text() == b""
        contig, rel = m.label_cells()
        assert contig.shape == (0, 3) and rel.shape == (0, 3)
        out = str(tmp_path / "empty.mums")
        m.write_label(out)
        assert open(out, "rb").read() == b"" and m.label_stats()["cells"] == 0


# ---- contigs -----------------------------------------------------------------------------------------------------------
def test_both_lookup_routes_in_one_call(engine):
    """1, 2, 1023, 1024, 1025 and 3000 contigs side by side: the last two are searched in HBM, the others from LDS"""
    counts = [1, 2, LDS_CONTIGS - 1, LDS_CONTIGS, LDS_CONTIGS + 1, 3000]
    t = M.make_rows(71, 900, 6, absent=0.05)
    contigs = M.make_contigs(72, t[3], counts, zero=0.1)
    want, stats = check(engine, t, contigs)
    assert stats["hbm_columns"] == 2
    for c in (2, 3, 4, 5):
        assert len(set(want[0][:, c].tolist())) > 200, c              # many contigs are hit
    check(engine, t, contigs, True)


def test_the_pool_of_a_batch_overflows(engine):
    """six columns of a full staging unit in one batch: the pool holds four, two go to HBM; a seventh column in the next batch of
    COLS columns is staged again"""
    counts = [LDS_CONTIGS] * 6 + [3] * (COLS - 6) + [LDS_CONTIGS]
    assert hbm_columns(counts) == 3 and hbm_columns(counts[:6]) == 2
    t = M.make_rows(73, 300, len(counts))
    contigs = M.make_contigs(74, t[3], counts)
    want, stats = check(engine, t, contigs)
    assert stats["hbm_columns"] == 3


def test_starts_on_every_boundary_and_beyond_32_bits(engine):
    """0, ends_k - 1, exactly ends_k, total - 1; column 1 lies above 2^32, column 2 near 2^40; contigs of length 0 around"""
    lens = [[0, 100, 0, 0, 50, 1000, 0], [(1 << 32) + 5, 0, 7, 1 << 20], [(1 << 40) - 3, 3, 0, 11, 0]]
    ends = [np.cumsum(x) for x in lens]
    rows = []
    for i in range(7):
        rows.append([int(ends[c][i % len(ends[c])]) for c in range(3)])               # exactly ends_k
        rows.append([int(ends[c][i % len(ends[c])]) - 1 for c in range(3)])           # ends_k - 1
    rows = [[s if 0 <= s < int(ends[c][-1]) else 0 for c, s in enumerate(r)] for r in rows]
    rows += [[0, 0, 0], [int(e[-1]) - 1 for e in ends], [7, 1 << 32, (1 << 40) - 4], [-1, (1 << 32) + 4, 1 << 40]]
    starts = np.array(rows, np.int64)
    table = (np.arange(1, len(rows) + 1, dtype=np.uint32) * 1234567, starts, np.ones(starts.shape, bool))
    table[1][2, 0] = 99
    names = [["c%d_%d" % (c, k) for k in range(len(x))] for c, x in enumerate(lens)]
    want, _ = check(engine, table, (names, lens))
    assert want[0][-3].tolist() == [5, 3, 3] and want[1][-3].tolist() == [999, (1 << 20) - 1, 10]       # total - 1
    assert want[0][-1].tolist() == [0, 0, 3] and want[1][-1].tolist() == [-1, (1 << 32) + 4, 0]
    assert (np.asarray(lens[0])[want[0][:, 0]][starts[:, 0] != -1] > 0).all()          # never a contig of length 0
    assert {len(str(v)) for v in want[1].ravel().tolist()} >= {1, 2, 3, 7, 10, 13}
    check(engine, table, (names, lens), True)


def test_absent_rows_and_columns(engine):
    t, contigs = rows_with_contigs(75, 3 * TILE, 7, absent=0.3)
    t[1][TILE] = -1                                          # a row of absent cells
    t[1][:, 3] = -1                                          # a column of them
    t[1][0] = -1
    t[1][-1] = -1
    want, stats = check(engine, t, contigs)
    assert stats["absent"] == int((t[1] == -1).sum()) > 3 * TILE + 7
    assert want[2].split(b"\n")[TILE].endswith(b"\t" + b",".join([b"0"] * 7) + b"\t" + b",".join([b"-1"] * 7))
    check(engine, t, contigs, True)


@pytest.mark.parametrize("name_len", [1, 200])
@pytest.mark.parametrize("n_docs", [3, 130])
def test_name_lengths(engine, n_docs, name_len):
    """names of one byte and of 200: with 130 columns a line is 26 KB, far more than the 64 bytes a wave deals out per step (the
    writer stages nothing in LDS: there is no span to exceed)"""
    t = M.make_rows(76, 70, n_docs, absent=0.1)
    contigs = M.make_contigs(77, t[3], [1 + c % 9 for c in range(n_docs)])
    contigs = ([[("%c" % (97 + (c + k) % 26)) * name_len for k in range(len(seq))] for c, seq in enumerate(contigs[0])], contigs[1])
    want, _ = check(engine, t, contigs, True, tag=(n_docs, name_len))
    assert (len(want[2]) // 70 > 26000) == (n_docs == 130 and name_len == 200)


def test_names_of_mixed_lengths_and_an_empty_one(engine):
    t = M.make_rows(78, 200, 70)
    contigs = M.make_contigs(79, t[3], [4] * 70)
    rng = np.random.default_rng(80)
    names = [["n%d_%d_" % (c, k) + "y" * int(rng.integers(0, 90)) for k in range(4)] for c in range(70)]
    names[69] = ["", "", "", ""]                             # (the last field of a line may be empty)
    names[5] = ["", "q", "", "r"]
    check(engine, t, (names, contigs[1]), True)


# ---- blocks ------------------------------------------------------------------------------------------------------------
def test_blocks_none_from_collinear_and_set_later(engine):
    import mumemto_amd
    t = collmodel.make_table(93, 300, 4, inversions=[(2, 40, 200)])
    with mumemto_amd.Merged.from_rows(engine, *t) as m:
        blk = m.collinear(1000)
        rows = [a.copy() for a in m.rows()]
        totals = (rows[1].max(axis=0) + 500).tolist()
        contigs = M.make_contigs(61, totals, [1, 4, 9, 30])
        assert len(blk) > 1
        want = M.label(rows[0], rows[1], rows[2], contigs, blk)
        assert m.label(contigs) == len(want[2]) and m.label_text() == want[2]
        # other blocks after label(): field 4 of the next text follows them, nothing else changes
        other = blk[1:]
        m.set_blocks(other)
        cells = m.label_cells()
        assert np.array_equal(cells[0], want[0]) and np.array_equal(cells[1], want[1])
        again = M.label(rows[0], rows[1], rows[2], contigs, other)[2]
        assert m.label_text() == again != want[2] and m.label_stats()["text_bytes"] == len(again)
        strip = lambda text: [l.split(b"\t")[:3] + l.split(b"\t")[4:] for l in text.split(b"\n")]      # noqa: E731
        assert strip(again) == strip(want[2])
    with mumemto_amd.Merged.from_rows(engine, *rows) as m:
        m.label(contigs)
        assert m.label_text() == M.label(rows[0], rows[1], rows[2], contigs)[2] and b"\t*\t" in m.label_text()
        m.set_blocks(blk)
        assert m.label_text() == want[2]


def test_pieces_give_the_same_bytes(engine, tmp_path):
    import mumemto_amd
    t, contigs = rows_with_contigs(81, 2000, 5, absent=0.1)
    want = M.label(t[0], t[1], t[2], contigs, None, True)[2]
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        assert m.label(contigs, True) == len(want) > 20 * 4096
        one, pieces = str(tmp_path / "one.mums"), str(tmp_path / "pieces.mums")
        m.write_label(one)
        os.environ["MMT_MERGED_TEXT_PIECE"] = "4096"
        try:
            m.write_label(pieces)
        finally:
            del os.environ["MMT_MERGED_TEXT_PIECE"]
        assert open(one, "rb").read() == want and open(pieces, "rb").read() == want
        assert not os.path.exists(one + ".tmp") and not os.path.exists(pieces + ".tmp")
        stats = m.label_stats()
        assert stats["write_ms"] > 0 and stats["lookup_ms"] > 0 and stats["text_bytes"] == len(want)
        with pytest.raises(mumemto_amd.MumemtoError, match="cannot write"):
            m.write_label(str(tmp_path / "no" / "such" / "dir.mums"))


# ---- the table and what hangs on it ------------------------------------------------------------------------------------
def test_refusals(engine):
    import mumemto_amd
    L = engine.L
    t, contigs = rows_with_contigs(51, 50, 3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)              # noqa: E731
    begin, lens, name_begin, blob = mumemto_amd.binding.contig_tables(contigs)
    blob = np.frombuffer(blob, np.uint8)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        # the accessors before label()
        a, b = C.c_void_p(), C.c_void_p()
        for rc in (L.mmt_merged_label_cells(m.h, None, None), L.mmt_merged_label_cells_device(m.h, C.byref(a), C.byref(b)),
                   L.mmt_merged_label_write_text(m.h, b"/dev/null")):
            assert rc == 3 and b"no labels attached" in L.mmt_last_error()
        assert L.mmt_merged_label_text(m.h, None) is None and b"no labels attached" in L.mmt_last_error()
        with pytest.raises(mumemto_amd.MumemtoError, match="no labels attached"):
            m.label_text()
        assert m.label_stats()["cells"] == 0
        # null tables
        assert L.mmt_merged_label(engine.h, m.h, None, None, None, None, 0, None) == 3 and b"contig_begin" in L.mmt_last_error()
        assert L.mmt_merged_label(engine.h, m.h, p(begin), None, None, None, 0, None) == 3 and b"contig_len" in L.mmt_last_error()
        assert L.mmt_merged_label(engine.h, m.h, p(begin), p(lens), None, None, 1, None) == 3 and b"name_begin" in L.mmt_last_error()
        assert L.mmt_merged_label(engine.h, m.h, p(begin), p(lens), p(name_begin), None, 1, None) == 3 and b"names" in L.mmt_last_error()
        assert L.mmt_merged_label(engine.h, m.h, p(begin), p(lens), None, None, 0, None) == 0       # names are not needed
        # the contigs
        empty = [0] * len(contigs[1][1])
        negative = list(contigs[1][2])
        negative[1] = -1
        for c, msg in (((contigs[0], [contigs[1][0], empty, contigs[1][2]]), "sequence 1 has total length 0"),
                       ((contigs[0], [contigs[1][0], contigs[1][1], negative]), "contig 1 of sequence 2 has the negative length -1"),
                       (([contigs[0][0], [], contigs[0][2]], [contigs[1][0], [], contigs[1][2]]), "sequence 1 has no contigs")):
            with pytest.raises(mumemto_amd.MumemtoError, match=msg):
                m.label(c)
            assert L.mmt_merged_label_cells(m.h, None, None) == 3            # a refused call attaches nothing
        with pytest.raises(mumemto_amd.MumemtoError, match="contigs of 2 sequences for a table of 3 columns"):
            m.label((contigs[0][:2], contigs[1][:2]))
        # a name that cannot be printed is refused where it is printed, and only there
        for ch in ("\t", "\n", ","):
            bad = ([list(seq) for seq in contigs[0]], contigs[1])
            bad[0][1][0] = "s1" + ch + "c0"
            with pytest.raises(mumemto_amd.MumemtoError, match="contig 0 of sequence 1 contains a tab, a newline or a comma"):
                m.label(bad, True)
            assert m.label(bad, False) > 0
        assert m.label(contigs, True) > 0


def test_a_start_at_or_beyond_the_total_is_refused_and_named(engine):
    import mumemto_amd
    t, contigs = rows_with_contigs(52, 3 * TILE, 40, counts=[1 + c % 7 for c in range(40)])
    totals = [sum(x) for x in contigs[1]]
    good = M.label(t[0], t[1], t[2], contigs)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        assert m.label(contigs) == len(good[2])
    for cells in ([(TILE + 3, 35, 0)], [(TILE + 3, 35, 1)], [(2 * TILE, 2, 5), (TILE + 3, 35, 1 << 40), (TILE + 3, 36, 0), (TILE + 4, 0, 0)]):
        starts = t[1].copy()
        for r, c, over in cells:
            starts[r, c] = totals[c] + over
        r, c, over = min(cells)
        with pytest.raises(M.OutOfRange) as ex:
            M.label(t[0], starts, t[2], contigs)
        assert (ex.value.row, ex.value.col) == (r, c)
        with mumemto_amd.Merged.from_rows(engine, t[0], starts, t[2]) as m:
            with pytest.raises(mumemto_amd.MumemtoError) as got:
                m.label(contigs)
            assert str(ex.value) in str(got.value), (str(got.value), str(ex.value))
            assert "the start %d of row %d, column %d" % (totals[c] + over, r, c) in str(got.value)
            assert engine.L.mmt_merged_label_cells(m.h, None, None) == 3 and m.label_stats()["cells"] == 0
            starts2 = np.ascontiguousarray(starts)
            assert all(np.array_equal(a, b) for a, b in zip(m.rows(), (t[0], starts2, t[2].astype(np.uint8))))


def test_label_reads_and_the_table_replacers_drop_it(engine):
    import mumemto_amd
    t = collmodel.make_table(94, 300, 4, inversions=[(2, 40, 200)])
    with mumemto_amd.Merged.from_rows(engine, *t) as m:
        blk = m.collinear(1000)
        calls = m.inversions()
        rows = [a.copy() for a in m.rows()]
        totals = (rows[1].max(axis=0) + 500).tolist()
        contigs = M.make_contigs(62, totals, [1, 4, 9, 30])
        covered = m.coverage(totals)
        runs = m.coverage_runs()
        n_bed = m.bed(contigs)
        bed = m.bed_records()
        assert len(blk) and len(calls) and n_bed
        want = M.label(rows[0], rows[1], rows[2], contigs, blk, True)
        assert m.label(contigs, True) == len(want[2]) and m.label_text() == want[2]
        # a pure reader: rows, blocks, calls, coverage and BED records are what they were
        assert all(np.array_equal(a, b) for a, b in zip(m.rows(), rows)) and np.array_equal(m.blocks(), blk)
        out = np.zeros((len(calls), 5), np.int64)
        assert engine.L.mmt_merged_inversion_calls(m.h, out.ctypes.data) == 0 and np.array_equal(out, calls)
        again = m.coverage_runs()
        assert np.array_equal(again[0], runs[0]) and np.array_equal(again[1], runs[1]) and covered.sum() > 0
        bed2 = m.bed_records()
        assert np.array_equal(bed2[0], bed[0]) and np.array_equal(bed2[1], bed[1])
        m.collinear(1000)
        assert engine.L.mmt_merged_label_cells(m.h, None, None) == 3 and m.label_stats()["cells"] == 0
        with pytest.raises(mumemto_amd.MumemtoError, match="no labels attached"):
            m.label_cells_device()
        assert m.label(contigs, True) == len(want[2])


def test_sort_like_direct_drops_the_labels():
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
            assert m.label(contigs) > 0
            assert eng.L.mmt_merged_sort_like_direct(eng.h, m.h) == 0
            assert eng.L.mmt_merged_label_cells(m.h, None, None) == 3
            length, off, st = m.rows()
            assert m.label(contigs) == len(M.label(length, off, st, contigs)[2]) and m.label_text() == M.label(length, off, st, contigs)[2]
    finally:
        eng.close()


def test_cells_in_hbm(engine):
    import torch
    import mumemto_amd
    from mumemto_amd.dist import DevicePointerView
    t, contigs = rows_with_contigs(66, 1000, 4, absent=0.1)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        m.label(contigs)
        contig, rel = m.label_cells()
        a, b = m.label_cells_device()
        assert a and b
        d_contig = torch.as_tensor(DevicePointerView(a, (1000, 4), "<i4"), device="cuda:0").cpu().numpy()
        d_rel = torch.as_tensor(DevicePointerView(b, (1000, 4), "<i8"), device="cuda:0").cpu().numpy()
        assert np.array_equal(d_contig.astype(np.uint32), contig) and np.array_equal(d_rel, rel)


def test_python_front_door():
    import mumemto_amd
    t, contigs = rows_with_contigs(67, 400, 3, absent=0.1)
    full = M.make_rows(68, 400, 3)
    blocks = bedmodel.make_blocks(69, 400)
    contigs_full = M.make_contigs(70, full[3], [2, 5, 11])
    for table, cont, blk, names in ((t, contigs, None, False), (full, contigs_full, blocks, True)):
        want = M.label(table[0], table[1], table[2], cont, blk, names)
        got = mumemto_amd.get_sequence_info(table[0], table[1], table[2], cont, blocks=blk, names=names)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
        assert got[0].dtype == np.uint32 and got[1].dtype == np.int64
