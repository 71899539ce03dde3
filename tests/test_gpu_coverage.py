"""GPU: the coverage (csrc/coverage.cpp, coverage_kernels.hip) against the stderr the reference's own tool printed
(tests/golden/coverage) and against the closed-form host model tests/covmodel.py, which tests/test_coverage_host.py holds to
the same files and to a naive bitmap.  Every comparison is exact: covered positions, run offsets and the runs themselves."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collmodel
import covmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "coverage")
RUNS = M.fixture_runs(GOLD)
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1")       # (the tool needs no tensor library: a quicker start)


def kernel_constant(name):
    text = open(os.path.join(ROOT, "mumemto_amd", "csrc", "coverage_kernels.hpp")).read()
    return int(re.search(r"%s\s*=\s*(\d+)" % name, text).group(1))


BLOCK = kernel_constant("SCAN_BLOCK")                    # elements of one round of a workgroup of the running maximum
TILE = BLOCK * kernel_constant("SCAN_ITEMS")             # elements of a workgroup: a tile
assert (BLOCK, TILE) == (256, 2048)


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def device(engine, table, seq_lengths, seq_idx=None, min_length=0):
    import mumemto_amd
    with mumemto_amd.Merged.from_rows(engine, *table[:3]) as m:
        covered = m.coverage(seq_lengths, seq_idx, min_length)
        return (covered,) + m.coverage_runs() + (m.coverage_stats(),)


def same(got, want, tag=""):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64 and got[2].dtype == np.int64
    assert np.array_equal(got[0], want[0]), (tag, got[0][:8], want[0][:8])
    assert np.array_equal(got[1], want[1]), (tag, got[1][:8], want[1][:8])
    assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2]), (tag, got[2][:4], want[2][:4])


def check(engine, table, seq_lengths, seq_idx=None, min_length=0, tag=""):
    want = M.coverage(table[0], table[1], seq_lengths, seq_idx, min_length)
    got = device(engine, table, seq_lengths, seq_idx, min_length)
    same(got, want, tag)
    stats = got[3]
    asked = table[1].shape[1] if seq_idx is None else 1
    assert stats["runs"] == len(want[2]), (tag, stats)
    assert stats["cols_sorted"] + stats["cols_ascending"] == (asked if len(table[0]) else 0), (tag, stats)
    return want, stats


def one_column(begins, lengths):
    begins = np.asarray(begins, np.int64).reshape(-1, 1)
    return np.asarray(lengths, np.uint32), begins, np.ones(begins.shape, bool)


@pytest.fixture(scope="module")
def wide():
    """one generator table of 94 columns (one of them absent throughout), shared and left unchanged"""
    t = M.make_table(31, 700, 94, absent_columns=(50,))
    return t, M.coverage(t[0], t[1], t[3])


# ---- the reference's own outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=[r["err"][:-4] for r in RUNS])
def test_golden_through_the_abi(engine, run):
    from mumemto_amd import mumsio
    from mumemto_amd.mum_coverage import parse_arguments
    args = parse_arguments(M.real_flags(run, GOLD))
    table = mumsio.read_rows(args.mumfile)
    seq_lengths = M.sequence_lengths(args.lens)
    want, _ = check(engine, table, seq_lengths, args.seq_idx, args.lenfilter, run["err"])
    got = device(engine, table, seq_lengths, args.seq_idx, args.lenfilter)
    assert M.stderr_line(args.seq_idx, got[0][args.seq_idx], seq_lengths[args.seq_idx]) == open(os.path.join(GOLD, run["err"]), "rb").read()


@pytest.mark.parametrize("name", ["synteny.s0", "synteny.s2", "partial.s4", "partial.s2.L200", "unsorted.s1", "overlap.s3",
                                  "overlap.s1.L200"])
def test_golden_through_the_tool(name, tmp_path):
    """`python -m mumemto_amd.mum_coverage` as a fresh child process: the reference's bytes on stderr, nothing on stdout, and
    the runs file; among the runs -s 0 of a .mums file, clipping at the end, a multi-FASTA lengths file, -i, a .bumbl, -L"""
    from mumemto_amd import mumsio
    from mumemto_amd.mum_coverage import parse_arguments
    run = [r for r in RUNS if r["err"] == name + ".err"][0]
    out = str(tmp_path / "runs.tsv")
    r = subprocess.run([sys.executable, "-m", "mumemto_amd.mum_coverage"] + M.real_flags(run, GOLD) + ["--runs", out], cwd=ROOT,
                       capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b"" and r.stderr == open(os.path.join(GOLD, run["err"]), "rb").read()
    args = parse_arguments(M.real_flags(run, GOLD))
    table = mumsio.read_rows(args.mumfile)
    _, _, runs = M.coverage(table[0], table[1], M.sequence_lengths(args.lens), args.seq_idx, args.lenfilter)
    assert open(out).read() == "".join("seq%d\t%d\t%d\n" % (args.seq_idx, b, e) for b, e in runs.tolist())
    assert not os.path.exists(out + ".tmp")


def test_all_sequences_through_the_tool(tmp_path):
    """--all: the lines of the five recorded single-sequence runs of `overlap`, in order, from one invocation"""
    out = str(tmp_path / "runs.tsv")
    r = subprocess.run([sys.executable, "-m", "mumemto_amd.mum_coverage", "-m", os.path.join(GOLD, "overlap.mums"), "--all",
                        "--runs", out], cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b"" and r.stderr == b"".join(open(os.path.join(GOLD, "overlap.s%d.err" % c), "rb").read() for c in range(5))
    from mumemto_amd import mumsio
    table = mumsio.read_rows(os.path.join(GOLD, "overlap.mums"))
    _, run_begin, runs = M.coverage(table[0], table[1], M.sequence_lengths(os.path.join(GOLD, "overlap.lengths")))
    want = "".join("seq%d\t%d\t%d\n" % (c, b, e) for c in range(5) for b, e in runs[int(run_begin[c]):int(run_begin[c + 1])].tolist())
    assert open(out).read() == want and len(runs) > 10


# ---- sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
def test_few_rows(engine, n):
    t = M.make_table(40, 2, 3)
    table = (t[0][:n], t[1][:n], t[2][:n])
    want, stats = check(engine, table, t[3], tag=n)
    if n == 0:
        assert (want[0] == 0).all() and (want[1] == 0).all() and stats["batches"] == 0 and stats["runs"] == 0


# the edges of a wave (64), of a round of a workgroup (BLOCK), of a tile (TILE = BLOCK x SCAN_ITEMS) and of two tiles, and the
# sizes the issue names; the extraction's own tile is 64 rows x 32 columns
# (TILE - 1, TILE, TILE + 1 and 2 TILE + 1 are 2047, 2048, 2049 and 4097)
@pytest.mark.parametrize("n", [63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1])
def test_tile_edges(engine, n):
    t = M.make_table(1000 + n, n, 3)
    _, stats = check(engine, t, t[3], tag=n)                # rows in random order: the sorted route
    assert stats["cols_sorted"] == 3
    order = np.argsort(t[1][:, 0], kind="stable")           # column 0 in order (absent cells first): the ascending route
    _, stats = check(engine, (t[0][order], t[1][order], t[2][order]), t[3], tag=(n, "in order"))
    assert stats["cols_ascending"] >= 1


def test_more_tiles_than_one_round_of_the_carry_kernel(engine):
    """the workgroup that scans the tile maxima takes BLOCK of them per round: BLOCK tiles and a few, one long early interval
    carried over all of them, runs on both sides of every boundary"""
    n = BLOCK * TILE + 4 * TILE + 5
    begins = np.arange(n, dtype=np.int64) * 10
    lengths = np.full(n, 9, np.uint32)                       # one apart: every row a run ...
    lengths[::7] = 10                                        # ... or touching the next
    lengths[3] = 10 * (BLOCK * TILE - 100)                   # covers up to 100 rows before the second round of the carry
    lengths[BLOCK * TILE + 10] = 10 * TILE                   # and one over the tile boundary behind it
    table = one_column(begins, lengths)
    want, stats = check(engine, table, [int(begins[-1]) + 5])       # (the last row is clipped)
    assert stats["cols_ascending"] == 1 and len(want[2]) > TILE


@pytest.mark.parametrize("n_docs", [1, 2, 33, 94, 130])
def test_column_counts(engine, n_docs, wide):
    if n_docs == 94:
        t, want = wide
        got = device(engine, t, t[3])
        same(got, want)
        assert want[0][50] == 0 and want[1][50] == want[1][51]
        return
    t = M.make_table(50 + n_docs, 300, n_docs)
    check(engine, t, t[3], tag=n_docs)


def test_all_columns_equal_the_single_column_calls(engine, wide):
    import mumemto_amd
    t, want = wide
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        for c in range(94):
            covered = m.coverage(t[3], c)
            run_begin, runs = m.coverage_runs()
            assert covered[c] == want[0][c] and covered.sum() == want[0][c], c
            assert run_begin[c] == 0 and (run_begin[c + 1:] == len(runs)).all(), c
            assert np.array_equal(runs, want[2][int(want[1][c]):int(want[1][c + 1])]), c


@pytest.mark.parametrize("batch", ["1", "7", "1000"])
def test_column_batches(engine, wide, batch):
    t, want = wide
    os.environ["MMT_COLLINEAR_BATCH"] = batch
    try:
        got = device(engine, t, t[3])
    finally:
        del os.environ["MMT_COLLINEAR_BATCH"]
    same(got, want, batch)
    assert got[3]["batches"] == {"1": 94, "7": 14, "1000": 1}[batch]


# ---- shapes ------------------------------------------------------------------------------------------------------------
def test_running_maximum_carried_across_many_tiles(engine):
    n = 5 * TILE + 37
    rng = np.random.default_rng(5)
    begins = np.sort(rng.integers(100, 10**6, n))
    lengths = rng.integers(1, 40, n).astype(np.uint32)
    begins[0], lengths[0] = 7, 900000                        # ends inside the fifth tile's values: nothing before it is a head
    table = one_column(begins, lengths)
    want, stats = check(engine, table, [10**6 + 20])
    assert stats["cols_ascending"] == 1 and want[2][0][0] == 7 and 900007 <= want[2][0][1] < 900100 and len(want[2]) > 10
    perm = rng.permutation(n)
    _, stats = check(engine, tuple(a[perm] for a in table), [10**6 + 20])
    assert stats["cols_sorted"] == 1


def test_all_equal_starts(engine):
    n = TILE + 100
    lengths = np.random.default_rng(6).integers(1, 500, n).astype(np.uint32)
    want, stats = check(engine, one_column(np.full(n, 12345), lengths), [10**6])
    assert want[0][0] == lengths.max() and want[2].tolist() == [[12345, 12345 + int(lengths.max())]]
    assert stats["cols_ascending"] == 1 and stats["cols_sorted"] == 0


def test_ascending_column_is_not_sorted_and_a_shuffled_one_is(engine):
    t = M.make_table(61, 3000, 2, absent=0.0)
    order = np.argsort(t[1][:, 0], kind="stable")
    table = (t[0][order], t[1][order], t[2][order])
    _, stats = check(engine, table, t[3], 0)
    assert (stats["cols_ascending"], stats["cols_sorted"]) == (1, 0) and stats["sort_ms"] == 0.0
    _, stats = check(engine, table, t[3])
    assert (stats["cols_ascending"], stats["cols_sorted"]) == (1, 1)
    _, stats = check(engine, t, t[3], 0)
    assert (stats["cols_ascending"], stats["cols_sorted"]) == (0, 1) and stats["sort_ms"] > 0.0


def test_starts_beyond_2_33_and_the_same_table_with_short_sequences(engine):
    t = M.make_table(62, 2500, 3, base=(1 << 33) + 12345)
    assert t[1][t[1] != -1].min() > 1 << 33
    want, _ = check(engine, t, t[3])
    assert (want[0] > 0).all() and (want[2] > 1 << 33).all()
    want, _ = check(engine, t, [1 << 33, 1000, 1])           # every row beyond the end
    assert (want[0] == 0).all() and len(want[2]) == 0


def test_min_length_at_equality(engine):
    t = M.make_table(63, 2500, 2)
    F = int(np.median(t[0]))
    assert (t[0] == F).any() and (t[0] == F - 1).any()
    a, _ = check(engine, t, t[3], None, F)
    b, _ = check(engine, t, t[3], None, F + 1)
    c, _ = check(engine, t, t[3], None, 0)
    assert (a[0] > b[0]).all() and (c[0] > a[0]).all()


def test_column_entirely_absent(engine):
    t = M.make_table(64, 2100, 3, absent_columns=(1,))
    want, _ = check(engine, t, t[3])
    assert want[0][1] == 0 and want[1][1] == want[1][2] and want[0][0] > 0 and want[0][2] > 0
    check(engine, t, t[3], 1)


# ---- the table and what hangs on it ------------------------------------------------------------------------------------
def test_table_blocks_and_calls_stay_and_new_blocks_drop_the_coverage(engine):
    import mumemto_amd
    t = collmodel.make_table(93, 300, 4, inversions=[(2, 40, 200)])
    with mumemto_amd.Merged.from_rows(engine, *t) as m:
        assert engine.L.mmt_merged_coverage_runs(m.h, None, None) == 3          # nothing attached yet
        with pytest.raises(mumemto_amd.MumemtoError, match="no coverage attached"):
            m.coverage_runs_device()
        blk = m.collinear(1000)
        calls = m.inversions()
        rows = [a.copy() for a in m.rows()]
        assert len(blk) and len(calls)
        seq_lengths = (rows[1].max(axis=0) + 200).tolist()
        same((m.coverage(seq_lengths),) + m.coverage_runs(), M.coverage(rows[0], rows[1], seq_lengths))
        assert all(np.array_equal(a, b) for a, b in zip(m.rows(), rows))
        assert np.array_equal(m.blocks(), blk)
        out = np.zeros((len(calls), 5), np.int64)
        assert engine.L.mmt_merged_inversion_calls(m.h, out.ctypes.data) == 0 and np.array_equal(out, calls)
        m.set_blocks(blk)                                    # (need not drop it)
        m.collinear(1000)
        assert engine.L.mmt_merged_coverage_runs(m.h, None, None) == 3 and m.coverage_stats()["runs"] == 0
        with pytest.raises(mumemto_amd.MumemtoError, match="no coverage attached"):
            m.coverage_runs()


def test_refusals(engine):
    import mumemto_amd
    t = M.make_table(65, 50, 3)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        for idx, lens, msg in ((3, t[3], "out of range"), (-2, t[3], "out of range"), (1, [5, 0, 5], "length 0"),
                               (None, [5, 5, -1], "length -1")):
            with pytest.raises(mumemto_amd.MumemtoError, match=msg):
                m.coverage(lens, idx)
        assert engine.L.mmt_merged_coverage(engine.h, m.h, None, 0, 0, None) == 3
        assert b"seq_lengths" in engine.L.mmt_last_error()
        assert m.coverage([5, 0, 5], 0)[0] <= 5              # a length that is not needed is not looked at


def test_runs_in_hbm(engine):
    import torch
    import mumemto_amd
    from mumemto_amd.dist import DevicePointerView
    t = M.make_table(66, 3000, 4)
    with mumemto_amd.Merged.from_rows(engine, *t[:3]) as m:
        m.coverage(t[3])
        run_begin, runs = m.coverage_runs()
        a, b = m.coverage_runs_device()
        assert a and b and len(runs) > 100
        d_begin = torch.as_tensor(DevicePointerView(a, (5,), "<i8"), device="cuda:0").cpu().numpy()
        d_runs = torch.as_tensor(DevicePointerView(b, (len(runs), 2), "<i8"), device="cuda:0").cpu().numpy()
        assert np.array_equal(d_begin.astype(np.uint64), run_begin) and np.array_equal(d_runs, runs)


def test_python_front_door():
    import mumemto_amd
    t = M.make_table(67, 400, 4)
    same(mumemto_amd.mum_coverage(t[0], t[1], t[2], t[3]), M.coverage(t[0], t[1], t[3]))
    same(mumemto_amd.mum_coverage(t[0], t[1], t[2], t[3], seq_idx=2, min_length=100), M.coverage(t[0], t[1], t[3], 2, 100))
