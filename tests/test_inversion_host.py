"""Host: the closed-form model of the inversion caller (tests/invmodel.py) and a pure-Python formatter against the stdout the
reference's own tool printed (tests/golden/inversion), the edges of the model, and the surface of the feature: header,
exports, binding, tool.

The fixtures are data only.  Tables: copies of tests/golden/collinear/*.mums, and collmodel.make_table tables `broken`
(inversions that gaps above the limit break into several blocks), `wide` (starts beyond 2^33, a minus column, a
multi-FASTA lengths file) and `shuffled` (rows in random order, partial rows, a move).  `broken.g1000.bumbl`, `wide.g200.mums`
and `inversion.g0.bumbl` carry blocks written by the reference's `collinear_block.py`.  Every `<run>.out` is the stdout of
`python <reference>/mumemto/find_inversions.py <flags of runs.json>` with the file names made absolute and AGPLIST replaced by
a file listing the paths under `agp`; the AGP files are written by hand around the two calls of `broken` at -g 1000."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collmodel
import invmodel as M
from mumemto_amd import binding

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "inversion")
RUNS = M.fixture_runs(GOLD)
ENTRY_POINTS = ("mmt_merged_set_blocks", "mmt_merged_inversions", "mmt_merged_inversion_calls",
                "mmt_merged_inversion_calls_device", "mmt_merged_inversion_stats")
TOOL = [sys.executable, "-m", "mumemto_amd.find_inversions"]


def tool_args(flags):
    from mumemto_amd.find_inversions import parse_arguments
    return parse_arguments(flags)


def test_fixture_set():
    """at least half of the recorded outputs hold a call, at least one holds none; every setting the issue names is there"""
    held = [open(os.path.join(GOLD, r["out"]), "rb").read().count(b"\n") - 1 for r in RUNS]
    assert held == [r["calls"] for r in RUNS]
    assert 2 * sum(k > 0 for k in held) >= len(held) and any(k == 0 for k in held)
    flags = [" ".join(r["flags"]) for r in RUNS]
    for want in ("-g 1000", "-g 0", "-g 200", "-L ", ".bumbl", "-a AGPLIST"):
        assert any(want in f for f in flags), want
    by_name = {r["out"]: r["calls"] for r in RUNS}
    assert (by_name["inversion.g1000.out"], by_name["inversion.g0.out"], by_name["partial.g1000.out"]) == (1, 0, 1)
    assert (by_name["minus_column.g1000.out"], by_name["minus_column.g0.out"], by_name["inversion.bumbl.out"]) == (2, 1, 0)
    for name in ("inversion", "partial", "minus_column", "synteny", "moved", "unsorted"):       # the copies are copies
        assert open(os.path.join(GOLD, name + ".mums"), "rb").read() == \
            open(os.path.join(HERE, "golden", "collinear", name + ".mums"), "rb").read()


@pytest.mark.parametrize("run", RUNS, ids=[r["out"][:-4] for r in RUNS])
def test_model_equals_the_reference_stdout(run, tmp_path):
    args = tool_args(M.real_flags(run, GOLD, tmp_path))
    table, _ = M.table_and_blocks(args.mumfile)
    collmodel.assert_no_ties(table[1])
    assert M.run_stdout(args) == open(os.path.join(GOLD, run["out"]), "rb").read()


def test_formatter_of_the_tool_equals_the_model(tmp_path):
    """mumemto_amd.find_inversions.format_calls + scaffold_breaks (host code of the tool) on the model's calls"""
    from mumemto_amd import find_inversions as tool
    for run in RUNS:
        args = tool_args(M.real_flags(run, GOLD, tmp_path))
        hap_ids = tool.sequence_names(args.filelist, args.chr)
        breaks = tool.scaffold_breaks(args.agp_filelist, args.chr, hap_ids) if args.scaffold else None
        got = tool.format_calls(M.run_calls(args), hap_ids, breaks, args.margin).encode()
        assert got == open(os.path.join(GOLD, run["out"]), "rb").read(), run["out"]


def chain_table(strand_of_block, order):
    return M.block_table([(order, strand_of_block)])


def test_model_edges():
    empty = (np.zeros(0, np.uint32), np.zeros((0, 3), np.int64), np.zeros((0, 3), bool))
    assert M.calls(*empty, np.zeros((0, 2), np.uint32)).shape == (0, 5)                        # B = 0
    t, blk = chain_table([False], [0])
    assert M.calls(*t, blk).shape == (0, 5)                                                     # B = 1: never a run
    t, blk = chain_table([False, False], [1, 0])
    # B = 2: the last row of block 1 (row 3) and the first row of block 0 (row 0)
    assert M.calls(*t, blk).tolist() == [[1, t[1][3, 1], t[1][0, 1] + t[0][0], 300, t[0][0]]]
    t, blk = chain_table([False, False], [0, 1])
    assert M.calls(*t, blk).shape == (0, 5)
    # one '+' block discards the whole run, it does not split it
    t, blk = chain_table([False, False, True, False, False], [4, 3, 2, 1, 0])
    assert M.calls(*t, blk).shape == (0, 5) and M.runs([4, 3, 2, 1, 0]) == [(0, 3)]
    # two runs separated by one non-decrease: 2 1 0 | 5 4 3
    order = [2, 1, 0, 5, 4, 3]
    t, blk = chain_table([False] * 6, order)
    got = M.calls(*t, blk)
    assert M.runs(order) == [(0, 1), (3, 4)] and got[:, 0].tolist() == [1, 1]
    assert got[0].tolist() == [1, t[1][5, 1], t[1][0, 1] + t[0][0], 500, t[0][0]]
    assert got[1].tolist() == [1, t[1][11, 1], t[1][6, 1] + t[0][6], 1100, 600 + t[0][6]]
    # -L exactly at the boundary
    spans = np.abs(got[:, 2] - got[:, 1])
    for L in (int(spans.min()), int(spans.max())):
        assert np.array_equal(M.calls(*t, blk, max_length=L), got[spans <= L]) and (spans == L).any()
        assert np.array_equal(M.calls(*t, blk, max_length=L - 1), got[spans < L])
    assert len(M.calls(*t, blk, max_length=int(spans.max()))) == 2 and len(M.calls(*t, blk, max_length=int(spans.min()) - 1)) == 0
    # a single reversed block is not a run
    t, blk = chain_table([True, False, True], [0, 1, 2])
    assert M.calls(*t, blk).shape == (0, 5)


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"MMT_API\s+int\s+%s\s*\(" % name, text), name
    assert re.search(r"mmt_merged_set_blocks\(mmt_engine\*\s*e,\s*mmt_merged\*\s*m,\s*const\s+uint32_t\*\s*lr,\s*uint64_t\s+n_blocks\)", text)
    assert re.search(r"mmt_merged_inversions\(mmt_engine\*\s*e,\s*mmt_merged\*\s*m,\s*int64_t\s+max_length,\s*uint64_t\*\s*n_calls\)", text)
    assert re.search(r"mmt_merged_inversion_stats\(const\s+mmt_merged\*\s*m,\s*double\s+out\[8\]\)", text)


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
    assert callable(mumemto_amd.find_inversions)
    for name in ("set_blocks", "inversions", "inversion_stats"):
        assert callable(getattr(mumemto_amd.Merged, name)), name
    import mumemto_amd.find_inversions as tool               # the tool's module takes the name over and stays callable
    assert callable(tool) and callable(mumemto_amd.find_inversions) and callable(tool.main)


def test_tool_help_refusals_and_failure_without_a_gpu(gpu_available, tmp_path):
    r = subprocess.run(TOOL + ["--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--input-prefix", "-i", "--mums", "-m", "--agp-filelist", "-a", "--filelist", "-f", "--chr", "-c", "--margin",
                 "-d", "--max-length", "-L", "--max-block-gap-len", "-g", "--verbose", "-v", "--device"):
        assert flag in r.stdout, flag
    r = subprocess.run(TOOL, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0                                     # one of -i / -m is required
    table = os.path.join(GOLD, "minus_column.mums")
    r = subprocess.run(TOOL + ["-m", table, "-a", str(tmp_path / "agp.txt")], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "must be provided together" in r.stderr and r.stdout == ""
    r = subprocess.run(TOOL + ["-m", table, "-c", "7"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "must be provided together" in r.stderr
    part = str(tmp_path / "part.mums")
    open(part, "w").write("30\t1,\t+,\n25\t,7\t,-\n")
    open(str(tmp_path / "part.lengths"), "w").write("a.fa 100\nb.fa 100\n")
    r = subprocess.run(TOOL + ["-m", part], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "No strict MUMs found after filtering. Aborting." in r.stderr and r.stdout == ""
    if gpu_available:
        return                                                   # (with a GPU: tests/test_gpu_inversion.py)
    r = subprocess.run(TOOL + ["-m", table], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr and r.stdout == ""
