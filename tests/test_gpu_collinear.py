"""GPU: collinear blocks of multi-MUMs (csrc/collinear.cpp, collinear_kernels.hip) against the golden files the reference's
own `collinear_block.main` wrote (tests/golden/collinear) and against the closed-form host model tests/collmodel.py, which
tests/test_collinear_host.py holds to the same golden files.  Every comparison is exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import collmodel as M
from mumemto_amd import mumsio, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "collinear")
TABLES = ("synteny", "inversion", "moved", "minus_column", "partial", "unsorted")
BUMBL = ("inversion", "unsorted")
RUNS = {"g1000": (1000, None), "g0": (0, None), "g200s150": (200, 150)}
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1")       # (the tool needs no tensor library: a quicker start)
RUN_FLAGS = {"g1000": ["-g", "1000"], "g0": ["-g", "0"], "g200s150": ["-g", "200", "--min-singleton-length", "150"]}


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def device_blocks(engine, table, max_break, single):
    """-> (filtered sorted rows, blocks, text) from the device path"""
    import mumemto_amd
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        blk = m.collinear(max_break, single)
        length, off, st = m.rows()
        return (length, off, st.astype(bool)), blk, m.text(), m.collinear_stats()


def check(engine, table, max_break=1000, single=None, tag=""):
    want_rows = M.prepare(*table)
    want = M.blocks(*want_rows, max_break=max_break, min_singleton_length=single)
    rows, blk, text, stats = device_blocks(engine, table, max_break, single)
    assert rows[1].shape == want_rows[1].shape, tag
    for got, ref in zip(rows, want_rows):
        assert np.array_equal(got, ref), tag
    assert blk.dtype == np.uint32 and blk.shape == want.shape and np.array_equal(blk, want), (tag, blk[:5], want[:5])
    assert text == M.mums_bytes(*want_rows, want), tag
    assert stats["rows_in"] == len(table[0]) and stats["rows_kept"] == len(want_rows[0]) and stats["n_blocks"] == len(want)
    return want_rows, want, stats


# ---- the reference's own outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
def test_golden_through_the_abi(engine, name, tmp_path):
    inputs = [name + ".mums"] + ([name + ".bumbl"] if name in BUMBL else [])
    for src in inputs:
        table = mumsio.read_rows(os.path.join(GOLD, src))
        for run, (g, s) in RUNS.items():
            rows, blk, text, _ = device_blocks(engine, table, g, s)
            gold_mums = os.path.join(GOLD, "%s.%s.mums" % (name, run))
            assert text == open(gold_mums, "rb").read(), (src, run)
            gold_rb = mumsio.read_mums(gold_mums, with_blocks=True)[3]
            assert np.array_equal(M.row_blocks(blk, len(rows[0])), gold_rb), (src, run)
            if name in BUMBL:
                out = str(tmp_path / "out.bumbl")
                mumsio.write_bumbl(out, rows[0], rows[1], rows[2], blocks=blk)
                assert open(out, "rb").read() == open(os.path.join(GOLD, "%s.%s.bumbl" % (name, run)), "rb").read(), (src, run)


@pytest.mark.parametrize("name,run,ext", [("synteny", "g1000", ".mums"), ("partial", "g200s150", ".mums"),
                                          ("unsorted", "g0", ".mums"), ("inversion", "g200s150", ".bumbl"),
                                          ("unsorted", "g1000", ".bumbl")])
def test_golden_through_the_tool(name, run, ext, tmp_path):
    """`python -m mumemto_amd.collinear_block` as a fresh child process: the same bytes as the reference's tool"""
    out = str(tmp_path / ("out" + ext))
    r = subprocess.run([sys.executable, "-m", "mumemto_amd.collinear_block", "-m", os.path.join(GOLD, name + ext), "-o", out]
                       + RUN_FLAGS[run], cwd=ROOT, capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(os.path.join(GOLD, "%s.%s%s" % (name, run, ext)), "rb").read()


def test_tool_default_name_replaced_field_and_refusals(tmp_path):
    """default output name <input>_sorted.<ext>; a fourth field on the input is replaced; a fifth is refused; a table with
    partial rows only writes nothing"""
    src = str(tmp_path / "again.mums")
    open(src, "wb").write(open(os.path.join(GOLD, "moved.g0.mums"), "rb").read())          # carries blocks of another run
    tool = [sys.executable, "-m", "mumemto_amd.collinear_block"]
    r = subprocess.run(tool + ["-i", str(tmp_path / "again")], cwd=ROOT, capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "again_sorted.mums"), "rb").read() == open(os.path.join(GOLD, "moved.g1000.mums"), "rb").read()
    five = str(tmp_path / "five.mums")
    open(five, "w").write("30\t1,2\t+,+\t0\textra\n")
    r = subprocess.run(tool + ["-m", five], cwd=ROOT, capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode != 0 and "extra fields" in r.stderr and not os.path.exists(str(tmp_path / "five_sorted.mums"))
    part = str(tmp_path / "part.mums")
    open(part, "w").write("30\t1,\t+,\n25\t,7\t,-\n")
    r = subprocess.run(tool + ["-m", part], cwd=ROOT, capture_output=True, text=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0 and "No strict MUMs found after filtering partial MUMs." in r.stderr
    assert not os.path.exists(str(tmp_path / "part_sorted.mums"))


# ---- seeded tables against the host model ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_tables(engine, n):
    for single in (None, 0):
        t = M.make_table(7, n, 3)
        check(engine, (t[0], t[1].reshape(n, 3), t[2].reshape(n, 3)), 1000, single, (n, single))


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_tile_edges(engine, n):
    """row counts around the tiles of the transpose (64), the sort and the scan; blocks that span those edges, an inversion
    across one, a moved segment across another"""
    t = M.make_table(n, n, 5, inversions=[(2, 60, 70), (3, 2040, min(2060, n - 1))], moves=[(1, 1000, 1030)],
                     gaps=(0, 40, 90), wide=(500, 1500, 1984, 2046))
    _, want, stats = check(engine, t, 1000, None, n)
    assert (want[:, 1] - want[:, 0]).max() > 64 and stats["cols_sorted"] == 3 and stats["cols_ascending"] == 2
    check(engine, t, 0, 300, n)


def test_the_only_descent_of_a_column_lies_across_a_tile_of_the_extraction(engine):
    """65 rows: row 64 is lane 0 of the second tile of the transpose and reads the key before it from the table; in column 2
    it lies in front of every other row, the column's only descent, so the column must be sorted and the last pair is cut"""
    lens, starts, strands = M.make_table(65, 65, 3, gaps=(0, 50), base=100000)
    starts[64, 2] = 5
    assert all(np.nonzero(np.diff(starts[:, c]) < 0)[0].tolist() == ([63] if c == 2 else []) for c in range(3))
    _, want, stats = check(engine, (lens, starts, strands), 1000)
    assert want.tolist() == [[0, 63]] and stats["cols_sorted"] == 1 and stats["cols_ascending"] == 2


def test_one_block_covers_every_row_and_none_at_all(engine):
    t = M.make_table(11, 4097, 3, gaps=(0, 50))
    _, want, _ = check(engine, t, 1000)
    assert want.tolist() == [[0, 4096]]
    lens, starts, strands = M.make_table(12, 300, 3, gaps=(0, 50))
    starts[:, 1] = starts[::-1, 1].copy()               # descending on '+': no pair agrees in this column
    _, want, _ = check(engine, (lens, starts, strands), 1000)
    assert len(want) == 0
    _, want, _ = check(engine, (lens, starts, strands), 1000, 100)
    assert len(want) == int((lens >= 100).sum())


@pytest.mark.parametrize("n_docs", [1, 2, 33, 94, 130])
def test_column_counts(engine, n_docs):
    """past a wave, 64 and 128 columns, and past an 8-bit count of agreeing columns"""
    last = n_docs - 1
    t = M.make_table(20 + n_docs, 300, n_docs, inversions=[(last, 100, 150)], moves=[(last // 2, 200, 240)], gaps=(0, 50),
                     wide=(30, 31, 129, 270))
    _, want, _ = check(engine, t, 1000, None, n_docs)
    assert len(want) == (6 if n_docs == 1 else 8)
    check(engine, t, 0, 150, n_docs)


def test_column_batches(engine):
    """the same answer when the columns go through in batches of three (the table does not fit beside its keys)"""
    t = M.make_table(31, 700, 8, inversions=[(7, 100, 150), (2, 300, 420)], moves=[(5, 500, 560)], partial=9, shuffle=True)
    _, _, stats = check(engine, t, 1000)
    assert stats["batches"] == 1
    os.environ["MMT_COLLINEAR_BATCH"] = "3"
    try:
        _, _, stats = check(engine, t, 1000)
        assert stats["batches"] == 3
    finally:
        del os.environ["MMT_COLLINEAR_BATCH"]


def test_forty_bit_keys_minus_column_partial_unsorted(engine):
    t = M.make_table(41, 500, 6, base=1 << 33, minus_cols=[2, 4], inversions=[(1, 50, 90), (4, 300, 330)])
    _, want, stats = check(engine, t, 1000)
    assert len(want) > 3 and stats["cols_sorted"] >= 3
    check(engine, t, 200, 150)
    # partial rows vanish, and a block closes over the place where they were
    t = M.make_table(42, 400, 4, gaps=(0, 50), partial=12)
    rows, want, _ = check(engine, t, 0)
    assert len(rows[0]) == 388 and want.tolist() == [[0, 387]]
    check(engine, t, 1000)
    # rows handed over in any order
    t = M.make_table(43, 600, 5, shuffle=True, partial=7, inversions=[(0, 100, 140)], moves=[(3, 400, 450)])
    _, want, stats = check(engine, t, 1000)
    assert stats["table_sorted"] and len(want) > 3


def chain(lens, gaps, plus, first):
    """starts of one column from the gaps between consecutive rows: ascending on '+', descending on '-'"""
    s = [first]
    for i, g in enumerate(gaps):
        s.append(s[-1] + int(lens[i]) + g if plus else s[-1] - int(lens[i + 1]) - g)
    return s


@pytest.mark.parametrize("max_break", [1, 200, 1000])
def test_gap_exactly_at_the_limit(engine, max_break):
    """a gap of exactly max_break keeps the pair, max_break + 1 cuts it, in a '+' column and in a '-' column"""
    lens = np.array([100, 37, 64, 250, 31, 90, 120, 45, 77], np.uint32)
    B = max_break
    g_plus = [B, B + 1, 0, B, 0, B + 1, 0, 0]
    g_minus = [0, 0, B, B + 1, B + 1, 0, B, 0]
    starts = np.stack([chain(lens, [0] * 8, True, 10), chain(lens, g_plus, True, 5000), chain(lens, g_minus, False, 10 ** 7)],
                      axis=1).astype(np.int64)
    strands = np.ones((9, 3), bool)
    strands[:, 2] = False
    M.assert_no_ties(starts)
    _, want, _ = check(engine, (lens, starts, strands), max_break)
    assert want.tolist() == [[0, 1], [2, 3], [6, 8]]
    _, want, _ = check(engine, (lens, starts, strands), 0)
    assert want.tolist() == [[0, 8]]


def test_singleton_length_at_equality(engine):
    t = M.make_table(51, 400, 4, inversions=[(2, 100, 130)])
    rows, plain, _ = check(engine, t, 200)
    alone = np.nonzero(M.row_blocks(plain, len(rows[0])) == M.NO_BLOCK)[0]
    s = int(np.sort(rows[0][alone])[len(alone) // 2])
    _, want, _ = check(engine, t, 200, s)
    singles = want[want[:, 0] == want[:, 1]][:, 0]
    assert set(singles.tolist()) == set(int(i) for i in alone if rows[0][i] >= s) and (rows[0][singles] == s).any()
    _, more, _ = check(engine, t, 200, s + 1)
    assert len(more) < len(want)


# ---- from a real run ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def haplotypes():
    return synth.pangenome(4, 50000, 0.01, seed=61, inversion=(2, 20000, 26000))


def test_rows_of_a_run_stay_on_the_device(engine):
    """strict run -> mmt_rows_mum_device -> mmt_merged_from_rows_device -> blocks == the host model on the same rows, with
    blocks before, inside and behind the inversion of haplotype 2; the fold of two anchor partitions of the same collection
    gives the same table and the same blocks"""
    import mumemto_amd
    docs = haplotypes()
    engine.set_docs(docs)
    engine.run()
    table = engine.rows_mum()
    table = (table[0].copy(), table[1].copy(), table[2].copy())
    want_rows = M.prepare(*table)
    M.assert_no_ties(want_rows[1])
    want = M.blocks(*want_rows, max_break=1000)
    with mumemto_amd.Merged.from_device(engine, *engine.rows_mum_device()) as m:
        blk = m.collinear(1000)
        length, off, st = m.rows()
        text = m.text()
    assert np.array_equal(length, want_rows[0]) and np.array_equal(off, want_rows[1]) and np.array_equal(st.astype(bool), want_rows[2])
    assert np.array_equal(blk, want) and text == M.mums_bytes(*want_rows, want)
    first = want[:, 0]
    minus = ~want_rows[2][first, 2]
    assert minus.any(), "no block inside the inversion"
    at = want_rows[1][first, 2]
    assert (~minus & (at < 20000)).any() and (~minus & (at > 26000)).any()
    parts = []
    for group in ([0, 1], [0, 2, 3]):
        engine.set_docs([docs[i] for i in group])
        engine.run(merge_metadata=True)
        L, o, s = engine.rows_mum()
        parts.append((L.copy(), o.copy(), s.copy(), engine.thresholds()[: len(docs[0][0]) + 1].copy()))
    with mumemto_amd.Merged.from_partitions(engine, parts) as m:
        blk2 = m.collinear(1000)
        length, off, st = m.rows()
    assert np.array_equal(off, want_rows[1]) and np.array_equal(length, want_rows[0])
    assert np.array_equal(blk2, want)


# ---- what does not change ----------------------------------------------------------------------------------------------
def test_text_without_blocks_is_unchanged(engine, tmp_path):
    """a handle that never saw mmt_merged_collinear formats three fields, byte for byte what mumsio.write_mums writes, and
    asking it for blocks is an error"""
    import mumemto_amd
    t = M.make_table(71, 333, 7, inversions=[(3, 30, 60)], shuffle=True)
    want = str(tmp_path / "want.mums")
    mumsio.write_mums(want, *t)
    with mumemto_amd.Merged.from_rows(engine, *t) as m:
        assert m.text() == open(want, "rb").read()
        with pytest.raises(mumemto_amd.MumemtoError):
            m.blocks_device()
        m.collinear(1000)
        assert m.text() != open(want, "rb").read() and m.blocks_device()[0]


def test_python_front_door():
    import mumemto_amd
    t = M.make_table(81, 150, 3, partial=4, shuffle=True)
    rows, blk = mumemto_amd.collinear_blocks(*t, max_break=200, min_singleton_length=150)
    want_rows = M.prepare(*t)
    assert all(np.array_equal(a, b) for a, b in zip(rows, want_rows))
    assert np.array_equal(blk, M.blocks(*want_rows, max_break=200, min_singleton_length=150))
