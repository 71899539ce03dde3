"""GPU: the inversion caller (csrc/inversion.cpp, inversion_kernels.hip) against the stdout the reference's own tool printed
(tests/golden/inversion) and against the closed-form host model tests/invmodel.py, which tests/test_inversion_host.py holds
to the same files.  Every comparison is exact."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collmodel
import invmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "inversion")
RUNS = M.fixture_runs(GOLD)
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1")       # (the tool needs no tensor library: a quicker start)


def kernel_constant(name):
    text = open(os.path.join(ROOT, "mumemto_amd", "csrc", "inversion_kernels.hpp")).read()
    return int(re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)" % name, text).group(1))


TILE = kernel_constant("MARK_THREADS") * kernel_constant("MARK_ITEMS")      # positions a workgroup of the mark pass takes
B = 3 * TILE + 37                                                           # three full tiles and a partial one


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def device_calls(engine, table, blk=None, max_block_gap=1000, max_length=None):
    """-> (calls, stats) from the device path: blocks given (set_blocks) or computed (collinear, no singletons)"""
    import mumemto_amd
    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        if blk is not None:
            m.set_blocks(blk)
            assert np.array_equal(m.blocks(), np.asarray(blk, np.uint32).reshape(-1, 2))
        else:
            m.collinear(max_block_gap, None)
        calls = m.inversions(max_length)
        return calls, m.inversion_stats()


def check(engine, table, blk, max_length=None, tag=""):
    counts = {}
    want = M.calls(*table, blk, max_length=max_length, counts=counts)
    got, stats = device_calls(engine, table, blk, max_length=max_length)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (tag, got[:4], want[:4])
    assert stats["n_blocks"] == len(blk) and stats["calls"] == len(want), (tag, stats)
    assert {k: stats[k] for k in counts} == counts, (tag, stats, counts)
    return want, stats


# ---- the reference's own outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=[r["out"][:-4] for r in RUNS])
def test_golden_through_the_abi(engine, run, tmp_path):
    from mumemto_amd.find_inversions import parse_arguments
    args = parse_arguments(M.real_flags(run, GOLD, tmp_path))
    table, blk = M.table_and_blocks(args.mumfile)
    got, _ = device_calls(engine, table, blk, args.max_block_gap, args.max_length)
    assert len(got) == run["calls"]
    hap_ids = M.sequence_names(args.filelist, args.chr)
    breaks = M.scaffold_breaks(args.agp_filelist, args.chr, hap_ids) if args.agp_filelist else None
    assert M.stdout_bytes(got, hap_ids, breaks, args.margin) == open(os.path.join(GOLD, run["out"]), "rb").read()


@pytest.mark.parametrize("name", ["minus_column.g1000", "broken.bumbl", "broken.g1000.chr", "wide.blocks", "shuffled.g1000",
                                  "inversion.g0"])
def test_golden_through_the_tool(name, tmp_path):
    """`python -m mumemto_amd.find_inversions` as a fresh child process: the same bytes as the reference's tool; among them a
    .bumbl with blocks, a .mums with a block field, the AGP columns, a lengths file of a multi-FASTA run, no call at all"""
    run = [r for r in RUNS if r["out"] == name + ".out"][0]
    r = subprocess.run([sys.executable, "-m", "mumemto_amd.find_inversions"] + M.real_flags(run, GOLD, tmp_path), cwd=ROOT,
                       capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == open(os.path.join(GOLD, run["out"]), "rb").read()
    carried = "bumbl" in name or "blocks" in name
    assert (b"Using pre-computed collinear blocks: " in r.stderr) == carried


# ---- tables whose blocks are given outright: the shapes the mark pass can get wrong ------------------------------------
def shaped_table():
    """one table, B blocks x 2 rows, a shape per column; the starts of columns 0 and 3 lie beyond 2^32"""
    minus, plus = np.zeros(B, bool), np.ones(B, bool)

    def column(segments, also_plus=()):
        order = M.reversed_segments(B, segments)
        strand = plus.copy()
        for a, b in segments:
            strand[order[a:b + 1]] = False
        strand[list(also_plus)] = True
        return order, strand

    cols = [
        column([(TILE - 6, TILE + 4), (2 * TILE - 1, 2 * TILE), (3 * TILE - 2, 3 * TILE + 1)]),   # runs across tile boundaries
        column([(0, 4), (B - 3, B - 1)]),                                                         # at position 0, up to B - 1
        (np.arange(B)[::-1].copy(), minus.copy()),                                                # one run over all blocks
        column([(0, B - 1)], also_plus=[B // 2]),                                                 # ... with one '+' block: none
        column([(10, 12), (13, 15), (TILE - 2, TILE - 1), (TILE, TILE + 1), (600, 601), (602, 640)]),   # adjacent runs
        (np.arange(B), plus.copy()),                                                              # ascending: skipped
        column([(20, 29)], also_plus=[]),                                                         # a reversed segment left on
    ]
    cols[6][1][:] = True                                                                          # ... '+': a run, no call
    return M.block_table(cols, bases=[1 << 33, 0, 0, 1 << 34, 0, 5, 0, 0])


@pytest.mark.parametrize("blocks", [65, 129])
def test_the_only_descent_of_a_column_lies_across_a_tile_of_the_extraction(engine, blocks):
    """the keys of the block heads leave the table 64 blocks a tile, and lane 0 of a tile reads the key before it from the
    table, through the block list: in column 2 the blocks 64 .. lie in front of block 0, so that its keys descend between
    blocks 63 and 64 and nowhere else (with 129 blocks the third tile begins on an ascent); the column must be sorted.
    Column 1 carries a reversed segment, and with it the calls"""
    rotated = np.concatenate([np.arange(64, blocks), np.arange(64)])
    minus_segment = np.ones(blocks, bool)
    minus_segment[10:21] = False
    table, blk = M.block_table([(M.reversed_segments(blocks, [(10, 20)]), minus_segment), (rotated, np.ones(blocks, bool))])
    heads = table[1][blk[:, 0].astype(np.int64), 2]
    assert np.nonzero(np.diff(heads) < 0)[0].tolist() == [63]
    want, stats = check(engine, table, blk, tag=blocks)
    assert len(want) == 1 and want[0][0] == 1
    assert stats["cols_sorted"] == 2 and stats["cols_ascending"] == 0 and stats["runs"] == 1


@pytest.fixture(scope="module")
def shaped(engine):
    table, blk = shaped_table()
    collmodel.assert_no_ties(table[1])
    want, stats = check(engine, table, blk, tag="shaped")
    return table, blk, want, stats


def test_shapes_against_the_model(shaped):
    table, blk, want, stats = shaped
    assert len(blk) == B >= 3 * TILE
    per_col = {c: int((want[:, 0] == c).sum()) for c in range(1, 8)}
    assert per_col == {1: 3, 2: 2, 3: 1, 4: 0, 5: 6, 6: 0, 7: 0}
    assert stats["cols_sorted"] == 6 and stats["cols_ascending"] == 1 and stats["runs"] == 3 + 2 + 1 + 1 + 6 + 1
    # the run over all blocks: last row of block B - 1 and first row of block 0, beyond 2^34 in the column, 2^33 in the anchor
    whole = want[want[:, 0] == 3][0]
    assert whole[1] > 1 << 34 and whole[3] > 1 << 33 and whole[3] == table[1][-1, 0] and whole[4] == table[1][0, 0] + table[0][0]


def test_max_length_at_the_boundary(engine, shaped):
    table, blk, want, _ = shaped
    spans = np.abs(want[:, 2] - want[:, 1])
    L = int(np.sort(spans)[len(spans) // 2])
    kept, _ = check(engine, table, blk, max_length=L, tag="L")
    assert 0 < len(kept) < len(want) and (np.abs(kept[:, 2] - kept[:, 1]) == L).any()
    fewer, _ = check(engine, table, blk, max_length=L - 1, tag="L - 1")
    assert len(fewer) < len(kept)
    none, stats = check(engine, table, blk, max_length=0, tag="0")
    assert len(none) == 0 and stats["runs"] == 14


def test_column_batches(engine, shaped):
    """the same calls when the columns go through one and two at a time"""
    table, blk, want, _ = shaped
    for batch in ("1", "2"):
        os.environ["MMT_COLLINEAR_BATCH"] = batch
        try:
            got, _ = device_calls(engine, table, blk)
        finally:
            del os.environ["MMT_COLLINEAR_BATCH"]
        assert np.array_equal(got, want), batch


def test_every_column_ascending(engine):
    cols = [(np.arange(B), np.ones(B, bool)), (np.arange(B), np.zeros(B, bool))]
    table, blk = M.block_table(cols)
    want, stats = check(engine, table, blk)
    assert len(want) == 0 and stats["cols_ascending"] == 2 and stats["cols_sorted"] == 0 and stats["sort_ms"] == 0.0


@pytest.mark.parametrize("n_blocks", [0, 1, 2])
def test_few_blocks(engine, n_blocks):
    table, blk = M.block_table([(np.arange(2)[::-1].copy(), np.zeros(2, bool))])
    blk = blk[:n_blocks]
    want, stats = check(engine, table, blk, tag=n_blocks)
    assert len(want) == (1 if n_blocks == 2 else 0) and stats["n_blocks"] == n_blocks
    if n_blocks < 2:
        assert stats["cols_sorted"] == 0 and stats["runs"] == 0
    # ... and tables too small to hold a block at all, through the collinear pass
    t = collmodel.make_table(7, n_blocks, 3)
    t = (t[0], t[1].reshape(n_blocks, 3), t[2].reshape(n_blocks, 3))
    got, stats = device_calls(engine, t)
    assert got.shape == (0, 5) and stats["n_blocks"] == 0


# ---- seeded tables through the collinear pass ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_block_gap", [1000, 0])
def test_seeded_table_through_collinear(engine, max_block_gap):
    """inversions that the gap limit breaks into hundreds of blocks, a minus column, partial rows, rows in random order"""
    t = collmodel.make_table(91, 4000, 5, inversions=[(2, 100, 2600), (4, 3000, 3900), (1, 2800, 2801)], minus_cols=[3],
                             partial=25, shuffle=True, base=1 << 32)
    rows = collmodel.prepare(*t)
    blk = collmodel.blocks(*rows, max_break=max_block_gap)
    want = M.calls(*rows, blk)
    got, stats = device_calls(engine, t, None, max_block_gap)
    assert np.array_equal(got, want) and stats["n_blocks"] == len(blk) and len(want) >= 1
    if max_block_gap:
        assert len(blk) >= 3 * TILE, len(blk)


def test_python_front_door():
    import mumemto_amd
    t = collmodel.make_table(92, 300, 4, inversions=[(2, 40, 200)], partial=5, shuffle=True)
    want = M.find(*t, max_block_gap=1000, max_length=None)
    assert len(want) >= 1
    assert np.array_equal(mumemto_amd.find_inversions(*t), want)
    span = int(np.abs(want[0, 2] - want[0, 1]))
    assert np.array_equal(mumemto_amd.find_inversions(*t, max_block_gap=1000, max_length=span - 1),
                          M.find(*t, max_block_gap=1000, max_length=span - 1))


# ---- refusals and what drops the calls ----------------------------------------------------------------------------------
def test_set_blocks_refusals(engine):
    import mumemto_amd
    table, blk = M.block_table([(np.arange(6)[::-1].copy(), np.zeros(6, bool))])
    n = len(table[0])

    def rc(m, blocks):
        lr = np.ascontiguousarray(blocks, np.uint32).reshape(-1, 2)
        return engine.L.mmt_merged_set_blocks(engine.h, m.h, lr.ctypes.data_as(C.c_void_p), len(lr))

    with mumemto_amd.Merged.from_rows(engine, *table) as m:
        for bad in ([[0, n]], [[3, 2]], [[0, 3], [3, 5]], [[4, 5], [0, 1]], [[0, 1], [0, 1]]):
            assert rc(m, bad) == 3 and b"ascending and disjoint" in engine.L.mmt_last_error(), bad
            with pytest.raises(mumemto_amd.MumemtoError):
                m.blocks_device()                                  # nothing was attached
        assert rc(m, blk) == 0 and rc(m, [[0, 0], [1, n - 1]]) == 0 and rc(m, np.zeros((0, 2), np.uint32)) == 0
    partial = (table[0], table[1].copy(), table[2])
    partial[1][3, 1] = -1
    with mumemto_amd.Merged.from_rows(engine, *partial) as m:
        assert rc(m, blk) == 3 and b"partial row" in engine.L.mmt_last_error()
    unsorted = (table[0], table[1].copy(), table[2])
    unsorted[1][[2, 3], 0] = unsorted[1][[3, 2], 0]
    with mumemto_amd.Merged.from_rows(engine, *unsorted) as m:
        assert rc(m, blk) == 3 and b"not ascending" in engine.L.mmt_last_error()
        with pytest.raises(mumemto_amd.MumemtoError, match="no collinear blocks"):
            m.inversions()


def test_new_blocks_drop_the_calls(engine):
    import mumemto_amd
    t = collmodel.make_table(93, 300, 4, inversions=[(2, 40, 200)])
    with mumemto_amd.Merged.from_rows(engine, *t) as m:
        with pytest.raises(mumemto_amd.MumemtoError, match="no collinear blocks"):
            m.inversions()
        with pytest.raises(mumemto_amd.MumemtoError, match="no inversion calls"):
            m.inversion_calls_device()
        blk = m.collinear(1000)
        first = m.inversions()
        assert len(first) >= 1 and m.inversion_calls_device() and np.array_equal(m.inversions(), first)      # recomputed
        m.collinear(1000)
        assert engine.L.mmt_merged_inversion_calls(m.h, None) == 3 and m.inversion_stats()["calls"] == 0
        assert np.array_equal(m.inversions(), first)
        m.set_blocks(blk)
        assert engine.L.mmt_merged_inversion_calls(m.h, None) == 3
        assert np.array_equal(m.inversions(), first)
