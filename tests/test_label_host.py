"""Host: the model of the contig labels (tests/labelmodel.py) against the files the reference's own tool wrote
(tests/golden/label, recorded by tests/golden/make_label.py) and against a plain per-cell loop, and the surface of the feature:
header, exports, binding, tool.  Every comparison is exact."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import labelmodel as M
from mumemto_amd import binding, mumsio
from mumemto_amd.find_inversions import blocks_of_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "label")
LABELLED = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "*.labeled.mums")) + glob.glob(os.path.join(GOLD, "*.named.mums")))
ENTRY_POINTS = ("mmt_merged_label", "mmt_merged_label_cells", "mmt_merged_label_cells_device", "mmt_merged_label_text",
                "mmt_merged_label_write_text", "mmt_merged_label_stats")
TOOL = [sys.executable, "-m", "mumemto_amd.get_sequence_info"]


def recorded(name):
    """a recorded file's name -> (table file, lengths file, names mode)"""
    m = re.fullmatch(r"(\w+?)((?:\.g\d+)?)\.(labeled|named)\.mums", name)
    return os.path.join(GOLD, m.group(1) + m.group(2) + ".mums"), os.path.join(GOLD, m.group(1) + ".lengths"), m.group(3) == "named"


def table_of(path):
    lengths, starts, strands, row_block = mumsio.read_mums(path, with_blocks=True)
    return lengths, starts, strands, None if row_block is None else blocks_of_rows(row_block)


def test_fixture_set():
    """the conditions the fixtures were chosen for, checked on the fixtures themselves"""
    assert len(LABELLED) == 2 * 9
    tables = {f: table_of(recorded(f)[0]) for f in LABELLED}
    no_blocks = [f for f, t in tables.items() if t[3] is None]
    assert sorted(no_blocks) == ["partial.labeled.mums", "partial.named.mums"]
    assert all((tables[f][1] == -1).any() for f in no_blocks)
    assert all(len(t[3]) for f, t in tables.items() if f not in no_blocks)           # no file with `-` on every row
    for f, t in tables.items():                                                      # no start at or beyond the total
        totals = [sum(x) for x in mumsio.read_contigs(recorded(f)[1])[1]]
        assert (t[1] < np.asarray(totals)[None, :]).all(), f
    names, lens = mumsio.read_contigs(os.path.join(GOLD, "minus_column.lengths"))
    t = tables["minus_column.g1000.labeled.mums"]
    for c, seq in enumerate(lens):
        assert seq[0] == 0 and 0 in seq[2:-1]
        assert set(np.cumsum(seq).tolist()) & set(t[1][:, c].tolist()), c           # a start exactly on a boundary
    text = open(os.path.join(GOLD, "partial.labeled.mums")).read()
    assert "274\t4068,-1,2295,1290,4691\t+,-,+,+,+\t*\t0,0,0,1,0\t4068,-1,2295,424,4691\n" in text


@pytest.mark.parametrize("name", LABELLED, ids=[f[:-5] for f in LABELLED])
def test_model_equals_the_reference_file(name):
    path, lens_path, named = recorded(name)
    lengths, starts, strands, blocks = table_of(path)
    contigs = mumsio.read_contigs(lens_path)
    want = open(os.path.join(GOLD, name), "rb").read()
    assert M.label(lengths, starts, strands, contigs, blocks, named)[2] == want
    assert M.loop_label(lengths, starts, strands, contigs, blocks, named) == want


# ---- the closed form, cell by cell ----------------------------------------------------------------------------------------
def with_zero_contigs(contigs):
    """contigs of length 0 at the start, in the middle and at the end of every sequence"""
    names = [["z_first"] + seq[:1] + ["z_mid", "z_mid2"] + seq[1:] + ["z_last"] for seq in contigs[0]]
    lens = [[0] + seq[:1] + [0, 0] + seq[1:] + [0] for seq in contigs[1]]
    return names, lens


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_plain_loop(seed):
    lengths, starts, strands, totals = M.make_rows(seed, 120 + 13 * seed, 4, absent=0.25 if seed % 2 else 0.0)
    contigs = with_zero_contigs(M.make_contigs(100 + seed, totals, [1, 2, 9, 70], zero=0.2))
    assert all(seq[0] == 0 and seq[-1] == 0 and 0 in seq[2:-1] for seq in contigs[1])
    blocks = None if seed < 2 else np.array([(0, 3), (10, 10), (len(lengths) - 5, len(lengths) - 1)], np.uint32)
    for named in (False, True):
        contig, rel, text = M.label(lengths, starts, strands, contigs, blocks, named)
        assert text == M.loop_label(lengths, starts, strands, contigs, blocks, named)
    assert contig.dtype == np.uint32 and rel.dtype == np.int64
    absent = starts == -1
    assert (contig[absent] == 0).all() and (rel[absent] == -1).all() and bool(absent.any()) == bool(seed % 2)
    for c in range(4):                                        # a contig of length 0 is never chosen
        assert (np.asarray(contigs[1][c])[contig[:, c][~absent[:, c]]] > 0).all()


def test_model_edges():
    lens = [[0, 10, 0, 90, 100]]
    starts = np.array([[0], [9], [10], [99], [100], [199], [-1]], np.int64)
    contig, rel = M.cells(starts, lens)
    assert contig[:, 0].tolist() == [1, 1, 3, 3, 4, 4, 0] and rel[:, 0].tolist() == [0, 9, 0, 89, 0, 99, -1]
    for bad in (200, 201, 1 << 40):
        with pytest.raises(M.OutOfRange) as ex:
            M.cells(np.array([[5, 5], [5, bad], [bad, 5]], np.int64), lens * 2)
        assert (ex.value.row, ex.value.col, ex.value.start, ex.value.total) == (1, 1, bad, 200)
        with pytest.raises(M.OutOfRange):
            M.loop_label([1, 1, 1], [[5, 5], [5, bad], [bad, 5]], [[1, 1]] * 3, ([["a"] * 5] * 2, lens * 2))
    one = (np.array([7], np.uint32), np.array([[-1, 150]], np.int64), np.array([[False, True]]))
    contigs = ([list("abcde")] * 2, lens * 2)
    assert M.label(*one, contigs)[2] == b"7\t-1,150\t-,+\t*\t0,4\t-1,50\n"
    assert M.label(*one, contigs, names=True)[2] == b"7\t-1,150\t-,+\t*\ta,e\t-1,50\n"
    assert M.label(*one, contigs, blocks=np.zeros((0, 2), np.uint32))[2] == b"7\t-1,150\t-,+\t-\t0,4\t-1,50\n"
    assert M.label(*one, contigs, blocks=np.array([[0, 0]]))[2] == b"7\t-1,150\t-,+\t0\t0,4\t-1,50\n"


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    sig = lambda s: re.search(r"\s*".join(re.escape(tok) for tok in s.split(" ")), text)      # noqa: E731
    assert sig("MMT_API int mmt_merged_label(mmt_engine* e, mmt_merged* m, const uint64_t* contig_begin, const int64_t* contig_len, "
               "const uint64_t* name_begin, const char* names, int use_names, uint64_t* text_bytes)")
    assert sig("MMT_API int mmt_merged_label_cells(const mmt_merged* m, uint32_t* contig, int64_t* rel)")
    assert sig("MMT_API int mmt_merged_label_cells_device(const mmt_merged* m, const uint32_t** contig, const int64_t** rel)")
    assert sig("MMT_API const char* mmt_merged_label_text(mmt_merged* m, size_t* len)")
    assert sig("MMT_API int mmt_merged_label_write_text(mmt_merged* m, const char* path)")
    assert sig("MMT_API int mmt_merged_label_stats(const mmt_merged* m, double out[8])")
    assert "mumemto/get_sequence_info.py" in text
    api = open(os.path.join(ROOT, "mumemto_amd", "csrc", "api.cpp")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, api), name
        assert name in binding.GPU_ABI_SYMBOLS, name


def test_sources_switch_and_documents():
    from mumemto_amd import build
    assert "label.cpp" in build.LIB_SOURCES and "label_kernels.hip" in build.LIB_SOURCES
    for f in ("label.cpp", "label.hpp", "label_kernels.hip", "label_kernels.hpp"):
        assert os.path.exists(os.path.join(ROOT, "mumemto_amd", "csrc", f)), f
    consts = open(os.path.join(ROOT, "mumemto_amd", "csrc", "label_kernels.hpp")).read()
    for name in ("LABEL_ROWS", "LABEL_COLS", "LABEL_LDS_UNITS"):
        assert re.search(r"%s\s*=\s*\d+" % name, consts), name
    assert "BED_LDS_CONTIGS" in consts
    hook = [l for l in open(os.path.join(ROOT, "mumemto_amd", "csrc", "switches.def")) if "MMT_MERGED_TEXT_PIECE" in l]
    assert len(hook) == 1 and "label" in hook[0]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "get_sequence_info" in open(os.path.join(ROOT, doc)).read(), doc


def test_python_surface():
    import mumemto_amd
    assert callable(mumemto_amd.get_sequence_info) and "get_sequence_info" in dir(mumemto_amd)
    for method in ("label", "label_cells", "label_cells_device", "label_text", "write_label", "label_stats"):
        assert callable(getattr(mumemto_amd.Merged, method)), method
    import mumemto_amd.get_sequence_info as tool             # the tool's module takes the name over and stays callable
    assert callable(tool) and callable(mumemto_amd.get_sequence_info) and callable(tool.main)
    begin, lens, name_begin, blob = binding.contig_tables(([["a\tb"]], [[5]]), check_names=False)     # the library judges
    assert blob == b"a\tb" and name_begin.tolist() == [0, 3]


def test_tool_arguments(tmp_path):
    from mumemto_amd.get_sequence_info import parse_arguments
    r = subprocess.run(TOOL + ["--help"], cwd=ROOT, capture_output=True, timeout=120)      # (argparse leaves before the library loads)
    assert r.returncode == 0
    for flag in (b"-m", b"--mumfile", b"-o", b"--output", b"-l", b"--lengths", b"-v", b"--verbose", b"-n", b"--contig-names",
                 b"--device"):
        assert flag in r.stdout, flag
    assert subprocess.run(TOOL, cwd=ROOT, capture_output=True, timeout=120).returncode == 2          # -m is required
    src = os.path.join(GOLD, "partial.mums")
    a = parse_arguments(["-m", src])
    assert (a.mumfile, a.lengths, a.output, a.verbose, a.contig_names) == \
        (src, os.path.join(GOLD, "partial.lengths"), os.path.join(GOLD, "partial_labeled.mums"), False, False)
    a = parse_arguments(["-m", os.path.join(GOLD, "partial"), "-n", "-v", "-o", "x.mums", "-l", os.path.join(GOLD, "moved.lengths")])
    assert (a.mumfile, a.lengths, a.output, a.verbose, a.contig_names) == (src, os.path.join(GOLD, "moved.lengths"), "x.mums", True, True)
    bumbl = tmp_path / "t.bumbl"
    bumbl.write_bytes(b"")
    (tmp_path / "t.lengths").write_text("/a.fa * 100\n/a.fa c 100\n")
    a = parse_arguments(["-m", str(tmp_path / "t")])          # the prefix of a .bumbl
    assert a.mumfile == str(bumbl) and a.output == str(tmp_path / "t_labeled.mums")
    for argv, msg in ((["-m", str(tmp_path / "none.mums")], b"MUM file %s not found." % str(tmp_path / "none.mums").encode()),
                      (["-m", str(tmp_path / "none")], b"MUM file %s not found." % str(tmp_path / "none").encode()),
                      (["-m", src, "-l", str(tmp_path / "none.lengths")],
                       b"Lengths file %s not found." % str(tmp_path / "none.lengths").encode())):
        r = subprocess.run(TOOL + argv, cwd=ROOT, capture_output=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr and r.stdout == b"", (argv, r.stderr)


def test_tool_refuses_a_plain_lengths_file(tmp_path):
    plain = tmp_path / "t.lengths"
    plain.write_text("/a.fa 100\n")
    mums = tmp_path / "t.mums"
    mums.write_text("30\t5\t+\n")
    r = subprocess.run(TOOL + ["-m", str(mums)], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip() == b"Multi-FASTA input required for contig ID annotation." and r.stdout == b""
    assert not os.path.exists(str(tmp_path / "t_labeled.mums"))
