"""Host: the closed-form model of the coverage (tests/covmodel.py) against the stderr the reference's own tool printed
(tests/golden/coverage) and against a naive bitmap, the edges of the model, and the surface of the feature: header, exports,
binding, tool.

The fixtures are data only.  Tables: copies of tests/golden/collinear/synteny.mums, partial.mums and unsorted.bumbl, and
`overlap.mums`, a covmodel.make_table table (overlapping, nested, duplicate and touching intervals, absent cells, rows over
and beyond the end, the last column absent throughout; its fourth sequence is 40 long).  `synteny.lengths` ends the third
sequence inside a row; `partial.lengths` is a multi-FASTA lengths file in the real form, contig lines of three fields.  Every
`<run>.err` is the stderr of `python <reference>/mumemto/mum_coverage.py <flags of runs.json>` with GOLD/ replaced by the
directory of the fixtures.  The reference imports numba, which was not installed where the fixtures were recorded: it ran
unchanged with a two-line stand-in package `numba` on PYTHONPATH whose `njit` returns its argument (njit only compiles, it
does not change what update_coverage means); the stand-in is not part of this repository."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import covmodel as M
from mumemto_amd import binding, mumsio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "coverage")
RUNS = M.fixture_runs(GOLD)
ENTRY_POINTS = ("mmt_merged_coverage", "mmt_merged_coverage_runs", "mmt_merged_coverage_runs_device",
                "mmt_merged_coverage_stats")
TOOL = [sys.executable, "-m", "mumemto_amd.mum_coverage"]


def tool_args(run):
    from mumemto_amd.mum_coverage import parse_arguments
    return parse_arguments(M.real_flags(run, GOLD))


def model_of_run(run, seq_lengths=None, min_length=None):
    """-> (covered, length of the sequence) of a recorded run by the closed form"""
    args = tool_args(run)
    lengths, starts, _ = mumsio.read_rows(args.mumfile)
    L = (seq_lengths or M.sequence_lengths(args.lens))[args.seq_idx]
    return M.column(lengths, starts[:, args.seq_idx], L, args.lenfilter if min_length is None else min_length)[0], L


def test_fixture_set():
    """the conditions the fixtures were chosen for, checked on the fixtures themselves"""
    errs = [open(os.path.join(GOLD, r["err"]), "rb").read() for r in RUNS]
    pct = []
    for run, err in zip(RUNS, errs):
        m = re.fullmatch(rb"seq(\d+): (\d+\.\d{3})%\n", err)
        assert m and int(m.group(1)) == tool_args(run).seq_idx, run
        pct.append(float(m.group(2)))
    assert 2 * sum(0 < p < 100 for p in pct) >= len(pct)
    assert b"seq3: 0.000%\n" in errs or b"seq4: 0.000%\n" in errs
    clipped = [r for r in RUNS if model_of_run(r)[0] != model_of_run(r, seq_lengths=[1 << 40] * 8)[0]]
    assert clipped and any(0 < model_of_run(r)[0] for r in clipped)
    filtered = [r for r in RUNS if tool_args(r).lenfilter and model_of_run(r)[0] != model_of_run(r, min_length=0)[0]]
    assert filtered and any(0 < model_of_run(r)[0] for r in filtered)
    args = [tool_args(r) for r in RUNS]
    for ext, idx in ((".mums", 0), (".mums", 2), (".mums", 4), (".bumbl", 0), (".bumbl", 3)):
        assert any(a.mumfile.endswith(ext) and a.seq_idx == idx for a in args), (ext, idx)
    last = {a.mumfile: mumsio.read_rows(a.mumfile)[1].shape[1] - 1 for a in args}
    assert all(any(a.mumfile == f and a.seq_idx == k for a in args) for f, k in last.items())
    for name in ("synteny.mums", "partial.mums", "unsorted.bumbl"):                       # the copies are copies
        assert open(os.path.join(GOLD, name), "rb").read() == open(os.path.join(HERE, "golden", "collinear", name), "rb").read()
    # the multi-FASTA lengths file: `PATH * total`, then contig lines of three fields
    lines = [l.split() for l in open(os.path.join(GOLD, "partial.lengths")).read().splitlines()]
    assert lines[0][1] == "*" and all(len(l) == 3 for l in lines) and sum(l[1] == "*" for l in lines) == 5
    assert M.sequence_lengths(os.path.join(GOLD, "partial.lengths")) == [int(l[2]) for l in lines if l[1] == "*"]


@pytest.mark.parametrize("run", RUNS, ids=[r["err"][:-4] for r in RUNS])
def test_model_equals_the_reference_stderr(run):
    covered, L = model_of_run(run)
    assert M.stderr_line(tool_args(run).seq_idx, covered, L) == open(os.path.join(GOLD, run["err"]), "rb").read()


def test_lengths_reader_and_formatter_of_the_tool_equal_the_model():
    from mumemto_amd import mum_coverage as tool
    for run in RUNS:
        args = tool_args(run)
        assert mumsio.read_seq_lengths(args.lens) == M.sequence_lengths(args.lens)
        covered, L = model_of_run(run)
        assert (tool.format_coverage(args.seq_idx, covered, L) + "\n").encode() == open(os.path.join(GOLD, run["err"]), "rb").read()


@pytest.mark.parametrize("seed,n,n_docs,F", [(1, 400, 4, 0), (2, 1500, 3, 0), (3, 700, 5, 150), (4, 60, 2, 0), (5, 900, 3, 2000)])
def test_model_equals_a_naive_bitmap(seed, n, n_docs, F):
    lengths, starts, _, seq_lengths = M.make_table(seed, n, n_docs, absent_columns=(n_docs - 1,) if seed == 3 else ())
    if seed == 4:
        seq_lengths[1] = 40                                                              # nearly every row beyond the end
    covered, run_begin, runs = M.coverage(lengths, starts, seq_lengths, None, F)
    some = False
    for c in range(n_docs):
        cov = M.bitmap(lengths, starts[:, c], int(seq_lengths[c]), F)
        assert int(covered[c]) == int(np.count_nonzero(cov)), c
        assert np.array_equal(runs[int(run_begin[c]):int(run_begin[c + 1])], M.runs_of_bitmap(cov)), c
        some |= 0 < covered[c] < seq_lengths[c]
    assert some or seed == 5
    one = M.coverage(lengths, starts, seq_lengths, 1, F)
    assert one[0][1] == covered[1] and one[0].sum() == covered[1] and len(one[2]) == run_begin[2] - run_begin[1]


def test_generator_has_the_shapes_it_promises():
    lengths, starts, _, seq_lengths = M.make_table(7, 2000, 4, absent_columns=(2,))
    ln = lengths.astype(np.int64)
    assert (starts[:, 2] == -1).all() and 0.05 < (starts[:, 0] == -1).mean() < 0.2
    present = starts[:, 0] != -1
    assert ((starts[:, 0] + ln > seq_lengths[0]) & (starts[:, 0] < seq_lengths[0]) & present).any()         # over the end
    assert (starts >= seq_lengths[None, :]).any()                                                            # at or beyond it
    both = present[1:] & present[:-1]
    assert (both & (starts[1:, 0] == starts[:-1, 0]) & (ln[1:] == ln[:-1])).any()                            # duplicates
    assert (both & (starts[1:, 0] == starts[:-1, 0] + ln[:-1])).any()                                        # touching
    b, e = M.intervals(lengths, starts[:, 0], int(seq_lengths[0]))
    top = np.maximum.accumulate(e)
    assert (e[1:] <= top[:-1]).any() and ((b[1:] < top[:-1]) & (e[1:] > top[:-1])).any()                     # nested, overlapping


def test_model_edges():
    L = 1000
    col = lambda rows, F=0, L=L: M.column(np.array([r[1] for r in rows], np.uint32), np.array([r[0] for r in rows], np.int64), L, F)
    runs = lambda rows, F=0, L=L: col(rows, F, L)[1].tolist()
    assert col([])[0] == 0 and runs([]) == []                                              # no rows
    assert col([(5, 10)])[0] == 10 and runs([(5, 10)]) == [[5, 15]]                        # one row
    assert col([(-1, 10), (-1, 20)])[0] == 0 and runs([(-1, 10), (-1, 20)]) == []          # all absent
    assert runs([(5, 10), (15, 10)]) == [[5, 25]] and col([(5, 10), (15, 10)])[0] == 20    # touching: one run
    assert runs([(5, 10), (16, 10)]) == [[5, 15], [16, 26]]                                # one apart: two runs
    assert runs([(16, 10), (5, 10)]) == [[5, 15], [16, 26]]                                # the order of the rows plays no part
    assert col([(990, 10)])[0] == 10 and runs([(990, 10)]) == [[990, 1000]]                # ending exactly at L
    assert col([(995, 10)])[0] == 5 and runs([(995, 10)]) == [[995, 1000]]                 # over the end: up to L
    assert col([(1000, 10)])[0] == 0 and runs([(1000, 10)]) == []                          # starting at L
    assert col([(1001, 10), (0, 3)])[0] == 3
    assert col([(5, 10), (40, 9)], F=10)[0] == 10 and col([(5, 10), (40, 9)], F=9)[0] == 19   # length == F kept, F - 1 dropped
    assert col([(0, 100), (10, 5), (10, 5), (50, 50)])[0] == 100                           # nested, duplicate, ending together
    assert runs([(0, 100), (10, 5), (200, 1)]) == [[0, 100], [200, 201]]                   # the run ends at the running maximum
    for seed in range(4):
        lengths, starts, _, seq_lengths = M.make_table(10 + seed, 500, 3)
        covered, run_begin, rr = M.coverage(lengths, starts, seq_lengths)
        for c in range(3):
            r = rr[int(run_begin[c]):int(run_begin[c + 1])]
            assert int((r[:, 1] - r[:, 0]).sum()) == int(covered[c])                       # sum(run lengths) == covered
            assert (r[:, 1] > r[:, 0]).all() and (r[1:, 0] > r[:-1, 1]).all()


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"MMT_API\s+int\s+%s\s*\(" % name, text), name
    sig = lambda s: re.search(r"\s*".join(re.escape(tok) for tok in s.split(" ")), text)
    assert sig("mmt_merged_coverage(mmt_engine* e, mmt_merged* m, const int64_t* seq_lengths, int64_t seq_idx, "
               "int64_t min_length, uint64_t* covered)")
    assert sig("mmt_merged_coverage_runs(const mmt_merged* m, uint64_t* run_begin, int64_t* runs)")
    assert sig("mmt_merged_coverage_runs_device(const mmt_merged* m, const uint64_t** run_begin, const int64_t** runs)")
    assert sig("mmt_merged_coverage_stats(const mmt_merged* m, double out[8])")


def test_library_exports_them_and_the_binding_lists_them():
    lib = ctypes.CDLL(binding.library_path())
    for name in ENTRY_POINTS:
        assert name in binding.GPU_ABI_SYMBOLS, name
        assert getattr(lib, name) is not None
    for name in binding.GPU_ABI_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.mmt_abi_version() == 7


def test_python_surface():
    import mumemto_amd
    assert callable(mumemto_amd.mum_coverage)
    for name in ("coverage", "coverage_runs", "coverage_runs_device", "coverage_stats"):
        assert callable(getattr(mumemto_amd.Merged, name)), name
    import mumemto_amd.mum_coverage as tool                  # the tool's module takes the name over and stays callable
    assert callable(tool) and callable(mumemto_amd.mum_coverage) and callable(tool.main)


def run_tool(flags):
    return subprocess.run(TOOL + flags, cwd=ROOT, capture_output=True, text=True)


def test_tool_help_and_refusals(tmp_path):
    r = run_tool(["--help"])
    assert r.returncode == 0
    for flag in ("--input-prefix", "-i", "--mums", "-m", "--lengths", "-l", "--len-filter", "-L", "--seq-idx", "-s", "--verbose",
                 "-v", "--device", "--all", "--runs"):
        assert flag in r.stdout, flag
    assert run_tool([]).returncode != 0                          # one of -i / -m is required
    table = os.path.join(GOLD, "synteny.mums")
    # both PREFIX.bumbl and PREFIX.mums
    for name in ("synteny.mums", "synteny.lengths"):
        shutil.copy(os.path.join(GOLD, name), str(tmp_path / name))
    lengths, starts, strands = mumsio.read_rows(table)
    mumsio.write_bumbl(str(tmp_path / "synteny.bumbl"), lengths, starts, strands)
    prefix = str(tmp_path / "synteny")
    r = run_tool(["-i", prefix])
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr == "Error: Both %s.bumbl and %s.mums exist. Please specify the file explicitly with --mums.\n" % (prefix, prefix)
    # -s out of range: the reference's message
    for idx in ("3", "-1", "17"):
        r = run_tool(["-m", table, "-s", idx])
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "Error: sequence index %s is out of range (0-2)\n" % idx), idx
    # an index the lengths file has and the table has not (the departure from the reference)
    r = run_tool(["-m", table, "-l", os.path.join(GOLD, "partial.lengths"), "-s", "4"])
    assert r.returncode == 1 and r.stdout == "" and "beyond the 3 sequences" in r.stderr
    r = run_tool(["-m", table, "-s", "1", "--all"])
    assert r.returncode != 0 and "not allowed with" in r.stderr and r.stdout == ""
    r = run_tool(["-m", str(tmp_path / "none.mums"), "-l", os.path.join(GOLD, "synteny.lengths")])
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("Error: ")


def test_tool_fails_without_a_gpu(gpu_available):
    if gpu_available:
        return                                                   # (with a GPU: tests/test_gpu_coverage.py)
    r = run_tool(["-m", os.path.join(GOLD, "synteny.mums")])
    assert r.returncode != 0 and "no CPU fallback" in r.stderr and r.stdout == ""
