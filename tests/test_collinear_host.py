"""Host: the closed-form model of the collinear blocks (tests/collmodel.py) against the files the reference's own
`collinear_block.main` wrote (tests/golden/collinear, made by tests/golden/make_collinear.py), the .mums / .bumbl readers and
writers of mumsio with block fields, and the surface of the feature: header, exports, binding, tool."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collmodel as M
from mumemto_amd import binding, mumsio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "collinear")
TABLES = ("synteny", "inversion", "moved", "minus_column", "partial", "unsorted")
BUMBL = ("inversion", "unsorted")
RUNS = {"g1000": (1000, None), "g0": (0, None), "g200s150": (200, 150)}
ENTRY_POINTS = ("mmt_merged_collinear", "mmt_merged_blocks", "mmt_merged_blocks_device", "mmt_merged_from_rows_device")


@pytest.mark.parametrize("name", TABLES)
def test_model_equals_the_reference_files(name, tmp_path):
    table = mumsio.read_mums(os.path.join(GOLD, name + ".mums"))
    M.assert_no_ties(table[1])
    rows = M.prepare(*table)
    assert len(rows[0]) >= 40 and (np.diff(rows[1][:, 0]) > 0).all() and not (rows[1] == -1).any()
    for run, (g, s) in RUNS.items():
        blk = M.blocks(*rows, max_break=g, min_singleton_length=s)
        assert len(blk) > 0 and (blk[:, 0] <= blk[:, 1]).all() and (blk[1:, 0] > blk[:-1, 1]).all()
        gold = os.path.join(GOLD, "%s.%s.mums" % (name, run))
        assert M.mums_bytes(*rows, blk) == open(gold, "rb").read(), run
        # ... and through mumsio: the reader returns rows and fourth field, the writer gives the bytes back
        gl, gs, gt, gb = mumsio.read_mums(gold, with_blocks=True)
        assert np.array_equal(gl, rows[0]) and np.array_equal(gs, rows[1]) and np.array_equal(gt, rows[2])
        assert np.array_equal(gb, M.row_blocks(blk, len(gl)))
        assert len(mumsio.read_mums(gold)) == 3
        out = str(tmp_path / "again.mums")
        mumsio.write_mums(out, gl, gs, gt, row_block=gb)
        assert open(out, "rb").read() == open(gold, "rb").read()
        if name in BUMBL:
            goldb = os.path.join(GOLD, "%s.%s.bumbl" % (name, run))
            assert M.bumbl_bytes(*rows, blk) == open(goldb, "rb").read(), run
            bl, bs, bt, bb = mumsio.read_bumbl(goldb, with_blocks=True)
            assert np.array_equal(bl, rows[0]) and np.array_equal(bs, rows[1]) and np.array_equal(bt, rows[2])
            assert bb.dtype == np.uint32 and np.array_equal(bb, blk)
            outb = str(tmp_path / "again.bumbl")
            mumsio.write_bumbl(outb, bl, bs, bt, blocks=bb)
            assert open(outb, "rb").read() == open(goldb, "rb").read()


def test_bumbl_input_equals_mums_input():
    for name in BUMBL:
        a = mumsio.read_mums(os.path.join(GOLD, name + ".mums"))
        b = mumsio.read_bumbl(os.path.join(GOLD, name + ".bumbl"), with_blocks=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b[:3])) and b[3] is None
    assert mumsio.read_mums(os.path.join(GOLD, "synteny.mums"), with_blocks=True)[3] is None


def test_model_edges():
    """the cases the closed form must get right by itself: no rows, one row, ties broken by row, a gap at the limit"""
    empty = (np.zeros(0, np.uint32), np.zeros((0, 3), np.int64), np.zeros((0, 3), bool))
    assert M.blocks(*M.prepare(*empty)).shape == (0, 2)
    one = (np.array([50], np.uint32), np.array([[5, 9]]), np.ones((1, 2), bool))
    assert M.blocks(*one).shape == (0, 2) and M.blocks(*one, min_singleton_length=50).tolist() == [[0, 0]]
    assert M.blocks(*one, min_singleton_length=51).shape == (0, 2)
    lens = np.array([10, 10, 10], np.uint32)
    starts = np.array([[0, 100], [30, 120], [60, 1130]])
    plus = np.ones((3, 2), bool)
    assert M.blocks(lens, starts, plus, max_break=1000).tolist() == [[0, 2]]           # 1130 - 120 - 10 = 1000: kept
    starts[2, 1] += 1
    assert M.blocks(lens, starts, plus, max_break=1000).tolist() == [[0, 1]]
    assert M.blocks(lens, starts, plus, max_break=0).tolist() == [[0, 2]]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"MMT_API\s+int\s+%s\s*\(" % name, text), name
    assert re.search(r"mmt_merged_collinear\(mmt_engine\*\s*e,\s*mmt_merged\*\s*m,\s*uint32_t\s+max_break,\s*int64_t\s+"
                     r"min_singleton_length,\s*uint64_t\*\s*n_blocks\)", text)


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
    assert callable(mumemto_amd.collinear_blocks) and callable(mumemto_amd.Merged.collinear)


def test_tool_help_and_failure_without_a_gpu(gpu_available, tmp_path):
    tool = [sys.executable, "-m", "mumemto_amd.collinear_block"]
    r = subprocess.run(tool + ["--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--input-prefix", "-i", "--mums", "-m", "--fout", "-o", "--max-gap-len", "-g", "--min-singleton-length", "-v"):
        assert flag in r.stdout, flag
    r = subprocess.run(tool, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0                                     # one of -i / -m is required
    five = str(tmp_path / "five.mums")
    open(five, "w").write("30\t1,2\t+,+\t0\textra\n")
    r = subprocess.run(tool + ["-m", five], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "extra fields" in r.stderr
    if gpu_available:
        return                                                   # (with a GPU: tests/test_gpu_collinear.py)
    out = str(tmp_path / "out.mums")
    r = subprocess.run(tool + ["-m", os.path.join(GOLD, "synteny.mums"), "-o", out], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr and not os.path.exists(out)
