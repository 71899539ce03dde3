"""GPU: the MEM density (csrc/density.cpp, density_kernels.hip) against the arrays the reference's own tool saved
(tests/golden/density) and against the closed-form host model tests/densmodel.py, which tests/test_density_host.py holds to
the same files and to a plain loop.  Every comparison is exact: the sums are integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import densmodel as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD_ENV = dict(os.environ, MUMEMTO_NO_TORCH="1")       # (the tool needs no tensor library: a quicker start)
TOOL = [sys.executable, "-m", "mumemto_amd.mem_density"]


@pytest.fixture(scope="module")
def engine():
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    yield eng
    eng.close()


def widths(size):
    return sorted({w for w in (1, 7, 64, size - 1, size, size + 5) if w >= 1})


def device(engine, rows, seq_lengths, W, cuts=()):
    """the table and the stats of `rows`, fed as the batches of whole rows that `cuts` (row numbers) divide them into"""
    import mumemto_amd
    lengths, occ_start, starts, docs = rows
    with mumemto_amd.Density(engine, seq_lengths, W) as d:
        edges = [0] + list(cuts) + [len(lengths)]
        for r0, r1 in zip(edges[:-1], edges[1:]):
            i, j = int(occ_start[r0]), int(occ_start[r1])
            d.add_rows(lengths[r0:r1], occ_start[r0:r1 + 1] - occ_start[r0], starts[i:j], docs[i:j])
        d.finish()
        return d.bins(), d.stats(), d.shape


def check(engine, rows, seq_lengths, W, cuts=(), tag=""):
    want = M.binned(*rows, seq_lengths, W)
    got, stats, shape = device(engine, rows, seq_lengths, W, cuts)
    size = int(max(seq_lengths))
    assert got.dtype == np.uint64 and got.shape == want.shape == (len(seq_lengths), M.nbins_of(size, W)), (tag, W, got.shape)
    assert shape == (len(seq_lengths), want.shape[1], size, min(W, size)), (tag, shape)
    assert np.array_equal(got, want), (tag, W, np.argwhere(got != want)[:4].tolist(), got[got != want][:4], want[got != want][:4])
    model = M.stats(*rows, seq_lengths)
    assert {k: stats[k] for k in model} == model, (tag, W, stats, model)
    return got


def rows_of(entries):
    """[(length, [(document, start), ...]), ...] -> the four arrays"""
    lengths = np.array([e[0] for e in entries], np.uint32)
    occ_start = np.concatenate(([0], np.cumsum([len(e[1]) for e in entries]))).astype(np.uint64)
    flat = [o for e in entries for o in e[1]]
    return lengths, occ_start, np.array([s for _, s in flat], np.int64), np.array([d for d, _ in flat], np.uint64)


# ---- the reference's own arrays ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.FIXTURES)
def test_golden_through_the_abi(engine, name):
    from mumemto_amd import mumsio
    mems, lens, npy = M.fixture_paths(name)
    gold = np.load(npy)
    seq_lengths = mumsio.read_seq_lengths(lens)
    rows = M.read_mems_plain(mems)
    got = check(engine, rows, seq_lengths, 1, tag=name)
    assert gold.dtype == np.float64 and np.array_equal(got.astype(np.float64), gold)
    for W in widths(gold.shape[1]):
        assert np.array_equal(check(engine, rows, seq_lengths, W, tag=name), M.sum_by_bins(gold.astype(np.int64), W)), (name, W)


@pytest.mark.parametrize("name", M.FIXTURES)
def test_golden_through_the_tool(name, tmp_path):
    """`python -m mumemto_amd.mem_density` as a fresh child process on a copy of the fixture: <stem>_coverage.npy beside the
    .mems file, equal to the reference's array in value, dtype and shape"""
    mems, lens, npy = M.fixture_paths(name)
    src = str(tmp_path / "run.mems")
    open(src, "wb").write(open(mems, "rb").read())
    r = subprocess.run(TOOL + ["-m", src, "-l", lens, "-v", "--max-occ", "7"], cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr.decode()
    got, gold = np.load(str(tmp_path / "run_coverage.npy")), np.load(npy)
    assert got.dtype == gold.dtype == np.float64 and got.shape == gold.shape and np.array_equal(got, gold)
    assert not os.path.exists(str(tmp_path / "run_coverage.npy.tmp")) and r.stdout == b""
    negative = int((M.read_mems_plain(mems)[2] < 0).sum())
    assert (b"Warning: %d of " % negative in r.stderr) == (negative > 0), r.stderr


def test_tool_bins_and_output(tmp_path):
    mems, lens, npy = M.fixture_paths("multifasta")
    out = str(tmp_path / "binned.npy")
    r = subprocess.run(TOOL + ["-m", mems, "-l", lens, "--bin", "64", "-o", out], cwd=ROOT, capture_output=True, timeout=120,
                       env=CHILD_ENV)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"", r.stderr.decode()
    got = np.load(out)
    want = M.sum_by_bins(np.load(npy).astype(np.int64), 64)
    assert got.dtype == np.float64 and got.shape == want.shape == (5, 24) and np.array_equal(got, want.astype(np.float64))
    assert not os.path.exists(out + ".tmp") and not os.path.exists(mems[:-5] + "_coverage.npy.tmp")


# ---- the model, shape by shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", [1, 2, 94])
@pytest.mark.parametrize("size", [1, 63, 64, 65, 1000])
def test_generator_rows(engine, size, num):
    """seeded rows with starts below 0, at size and beyond it, and ends exactly at size, at every bin width of the issue"""
    rows = M.make_rows(seed=1000 * num + size, n_rows=60, num=num, size=size)
    seq_lengths = np.full(num, max(1, size // 2), np.int64)
    seq_lengths[num // 2] = size                       # (the others are shorter: the cut is at size all the same)
    for W in widths(size):
        check(engine, rows, seq_lengths, W, tag="size %d num %d" % (size, num))


@pytest.mark.parametrize("size", [100, 95])
def test_intervals_on_bin_edges(engine, size):
    """W = 10 over size 100 (W divides it: an end at size would be bin 10, which does not exist) and 95 (the last bin is
    short): intervals that begin on an edge, end on one, lie inside one bin, span three bins, end at size -- the case
    without an end event -- begin at size - 1, cover everything, and one per bin"""
    entries = [(10, [(0, 20), (1, 20)]),                  # begins and ends on an edge
               (7, [(0, 30), (1, 33)]),                   # begins on an edge; ends on one
               (3, [(0, 41), (1, 46)]),                   # inside one bin
               (25, [(0, 12), (1, 58)]),                  # three bins and a part of a fourth
               (21, [(0, 19), (1, 29)]),                  # one position of a bin, two whole bins
               (size - 60, [(0, 60), (1, 60)]),           # ends at size
               (1, [(0, size - 1), (1, size - 1)]),       # the last position
               (size, [(0, 0), (1, 0)]),                  # everything
               (5, [(k & 1, 10 * k) for k in range((size + 9) // 10)])]
    rows = rows_of(entries)
    for W in (10, 1, 3, size):
        got = check(engine, rows, [size, size], W, tag="edges")
    assert got.tolist() == M.per_base(*rows, [size, size]).sum(axis=1, keepdims=True).tolist()


@pytest.mark.parametrize("spread", [False, True], ids=["piled", "spread"])
def test_pile_ups_count_exactly(engine, spread):
    """rows of 2, 64, 65, 300 and 5000 occurrences, all on one position of one sequence or spread evenly over three: more
    lanes than a wave and more than a workgroup add to one destination, and the count is exact"""
    size, counts = 1000, (2, 64, 65, 300, 5000)
    entries = []
    for n in counts:
        if spread:
            entries.append((9, [(k % 3, (k * 37) % (size - 9)) for k in range(n)]))
        else:
            entries.append((9, [(1, 495)] * n))
    rows = rows_of(entries)
    for W in (1, 7, 64, size):
        got = check(engine, rows, [size, size, 640], W, tag="pile")
    assert int(got.sum()) == 9 * sum(counts)
    if not spread:
        assert check(engine, rows, [size, size, 640], 1)[1, 495:504].tolist() == [sum(counts)] * 9


def test_batches_of_whole_rows(engine):
    """a 6-row table as one batch, cut in two at every row boundary, and row by row"""
    rows = M.make_rows(seed=6, n_rows=6, num=3, size=500, occ=(2, 70))
    seq_lengths = [500, 300, 420]
    for W in (1, 64):
        whole = check(engine, rows, seq_lengths, W, tag="one batch")
        for cut in range(1, 6):
            assert np.array_equal(check(engine, rows, seq_lengths, W, cuts=(cut,), tag="cut %d" % cut), whole)
        assert np.array_equal(check(engine, rows, seq_lengths, W, cuts=(1, 2, 3, 4, 5), tag="row by row"), whole)


def test_rows_without_occurrences(engine):
    """occ_start may repeat a value: such a row has no occurrences, and the row behind it is found all the same"""
    rows = rows_of([(5, []), (7, [(0, 3), (0, 50)]), (9, []), (9, []), (11, [(0, 20)]), (2, [])])
    check(engine, rows, [64], 1, tag="empty rows")
    check(engine, rows, [64], 16, tag="empty rows")


def test_empty_table_and_add_after_finish(engine):
    import mumemto_amd
    none = rows_of([])
    assert not check(engine, none, [10, 7], 1, tag="no rows").any()
    first, second = M.make_rows(seed=8, n_rows=9, num=2, size=200), M.make_rows(seed=9, n_rows=5, num=2, size=200)
    with mumemto_amd.Density(engine, [200, 150], 7) as d:
        with pytest.raises(mumemto_amd.MumemtoError, match="no table yet"):
            d.bins()
        d.finish()
        assert not d.bins().any()                                        # a table without rows: all zero
        d.add_rows(*first)
        with pytest.raises(mumemto_amd.MumemtoError, match="no table yet"):
            d.bins_device()
        d.finish()
        assert np.array_equal(d.bins(), M.binned(*first, [200, 150], 7))
        d.finish()                                                       # (finishing twice changes nothing)
        assert np.array_equal(d.bins(), M.binned(*first, [200, 150], 7))
        d.add_rows(*second)
        d.add_rows(*none)
        d.finish()
        assert np.array_equal(d.bins(), M.binned(*first, [200, 150], 7) + M.binned(*second, [200, 150], 7))
        stats = d.stats()
        assert stats["occurrences"] == len(first[2]) + len(second[2]) and stats["add_ms"] > 0 and stats["finish_ms"] > 0
        assert d.bins_device()[0] and d.bins_device()[1:] == (2, 29)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    import ctypes as C
    import mumemto_amd
    from mumemto_amd.binding import MumemtoError
    L = engine.L
    with pytest.raises(MumemtoError, match="rc=3.*no sequences"):
        mumemto_amd.Density(engine, [], 1)
    with pytest.raises(MumemtoError, match="rc=3.*sequence 1 has length 0"):
        mumemto_amd.Density(engine, [5, 0, 7], 1)
    with pytest.raises(MumemtoError, match="rc=3.*sequence 0 has length -4"):
        mumemto_amd.Density(engine, [-4], 1)
    with pytest.raises(MumemtoError, match="rc=3.*bin width of 0"):
        mumemto_amd.Density(engine, [5], 0)
    h = C.c_void_p()
    assert L.mmt_density_create(engine.h, None, 3, 1, C.byref(h)) == 3 and b"seq_lengths must hold" in L.mmt_last_error()
    assert not h.value
    # 94 sequences of 2^40 positions, a bin each: 24 x 94 x 2^40 bytes
    with pytest.raises(MumemtoError, match=r"rc=3.*exceed the \d+ bytes the device heap can give; the smallest --bin that fits is \d+"):
        mumemto_amd.Density(engine, [1 << 40] * 94, 1)
    good = rows_of([(5, [(0, 1), (1, 2)]), (6, [(1, 3), (0, 4)])])
    with mumemto_amd.Density(engine, [50, 40], 1) as d:
        bad = (good[0], good[1], good[2], np.array([0, 1, 2, 0], np.uint64))
        with pytest.raises(MumemtoError, match="rc=3.*row 1 has an occurrence in sequence 2, but there are 2 sequences"):
            d.add_rows(*bad)
        with pytest.raises(MumemtoError, match="rc=3.*occ_start is not ascending at row 1"):
            d.add_rows(good[0], np.array([0, 3, 2], np.uint64), good[2], good[3])
        with pytest.raises(MumemtoError, match="rc=3.*occ_start must begin at 0"):
            d.add_rows(good[0], np.array([1, 2, 4], np.uint64), good[2], good[3])
        huge = np.array([0, (1 << 40) + 1], np.uint64)
        assert L.mmt_density_add_rows(d.h, good[0].ctypes.data_as(C.c_void_p), huge.ctypes.data_as(C.c_void_p),
                                      good[2].ctypes.data_as(C.c_void_p), good[3].ctypes.data_as(C.c_void_p), 1) == 3
        assert b"beyond 2^40" in L.mmt_last_error()
        assert L.mmt_density_add_rows(d.h, None, None, None, None, 2) == 3 and b"null row tables" in L.mmt_last_error()
        assert L.mmt_density_add_rows(d.h, good[0].ctypes.data_as(C.c_void_p), good[1].ctypes.data_as(C.c_void_p), None, None, 2) == 3
        assert b"null occurrence tables" in L.mmt_last_error()
        # nothing was launched by any of them, and the tables are as they were
        d.add_rows(*good)
        d.finish()
        assert np.array_equal(d.bins(), M.binned(*good, [50, 40], 1))
    assert engine.L.mmt_abi_version() == 7                        # (callers detect the entry points by their symbols)


def test_engine_rows_in_hbm(engine, tmp_path, monkeypatch):
    """Engine.run in MEM mode on a small seeded collection: the density of the rows where the run left them against the model
    on rows_mem(), and against the tool on the run's .mems text; then the refusals of add_engine"""
    import mumemto_amd
    from mumemto_amd import synth
    from mumemto_amd.binding import MumemtoError
    docs = synth.pangenome(5, 3000, 0.02, seed=44, indel_rate=0.001, tandem=(2, 500, 560, 2))
    seq_lengths = [sum(len(r) for r in d) for d in docs]
    engine.set_docs(docs)
    engine.run(min_match_len=12, num_distinct=4, max_doc_freq=3)
    lengths, occ_start, starts, ids, _ = engine.rows_mem()
    rows = (lengths, occ_start, starts, ids)
    assert len(lengths) > 20 and len(starts) > 2 * len(lengths) - 1
    for W in (1, 100, max(seq_lengths)):
        got = engine.mem_density(seq_lengths, W)
        assert got.dtype == np.uint64 and np.array_equal(got, M.binned(*rows, seq_lengths, W)), W
    assert np.array_equal(engine.mem_density(seq_lengths), M.per_base(*rows, seq_lengths).astype(np.uint64))
    with mumemto_amd.Density(engine, seq_lengths, 100) as d:            # a host batch and the rows in HBM into one table
        d.add_engine()
        d.add_rows(*rows)
        d.finish()
        assert np.array_equal(d.bins(), 2 * M.binned(*rows, seq_lengths, 100))
        assert d.stats()["occurrences"] == 2 * len(starts)
    # the tool on the text of the same run
    mems, lens = str(tmp_path / "run.mems"), str(tmp_path / "run.lengths")
    open(mems, "wb").write(engine.output_text())
    open(lens, "w").write("".join("/data/doc%d.fa %d\n" % (c, v) for c, v in enumerate(seq_lengths)))
    r = subprocess.run(TOOL + ["-m", mems, "-l", lens], cwd=ROOT, capture_output=True, timeout=120, env=CHILD_ENV)
    assert r.returncode == 0, r.stderr.decode()
    assert np.array_equal(np.load(str(tmp_path / "run_coverage.npy")), M.per_base(*rows, seq_lengths).astype(np.float64))
    # refusals: another number of sequences; a MUM-mode run; a run whose sink dropped the rows
    with mumemto_amd.Density(engine, seq_lengths + [10], 1) as d:
        with pytest.raises(MumemtoError, match="rc=3.*6 sequence lengths, but the engine's last run had 5 documents"):
            d.add_engine()
    engine.run(min_match_len=12)
    with mumemto_amd.Density(engine, seq_lengths, 1) as d:
        with pytest.raises(MumemtoError, match="rc=3.*MUM mode"):
            d.add_engine()
        d.add_rows(*rows)                                                # the engine and the tables stay usable
        d.finish()
        assert np.array_equal(d.bins(), M.binned(*rows, seq_lengths, 1))
    monkeypatch.setenv("MMT_SINK_DISCARD", "1")
    engine.set_producer("pfp")
    try:
        engine.set_text_sink(str(tmp_path / "sunk.mems"))
        engine.set_docs(docs)
        engine.run(min_match_len=12, num_distinct=4, max_doc_freq=3)
        engine.set_text_sink(None)
        assert open(str(tmp_path / "sunk.mems"), "rb").read() == open(mems, "rb").read()
        with mumemto_amd.Density(engine, seq_lengths, 1) as d:
            with pytest.raises(MumemtoError, match="rc=3.*kept no rows"):
                d.add_engine()
    finally:
        engine.set_text_sink(None)
        engine.set_producer("auto")
