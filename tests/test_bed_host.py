"""Host: the closed-form model of the BED writer (tests/bedmodel.py) against the files the reference's own tool wrote
(tests/golden/bed, recorded by tests/golden/make_bed.py) and against a plain per-record loop, the reader of the contig table,
and the surface of the feature: header, exports, binding, tool.

A recorded file of a table that ends in a block lacks that block's line (the reference never flushes it): there the model
with drop_open_tail equals the file, and the model without it adds exactly one line."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bedmodel as M
from mumemto_amd import binding, mumsio
from mumemto_amd.find_inversions import blocks_of_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "bed")
BEDS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "*.bed")))
ENTRY_POINTS = ("mmt_merged_bed", "mmt_merged_bed_records", "mmt_merged_bed_records_device", "mmt_merged_bed_text",
                "mmt_merged_bed_write_text", "mmt_merged_bed_stats")
TOOL = [sys.executable, "-m", "mumemto_amd.mum_to_bed"]


def recorded(bed):
    """a recorded file's name -> (table file, lengths file, seq_idx, min_singleton_length)"""
    m = re.fullmatch(r"(\w+?)((?:\.g\d+)?)\.s(\d+)\.L(\d+)\.bed", bed)
    return (os.path.join(GOLD, m.group(1) + m.group(2) + ".mums"), os.path.join(GOLD, m.group(1) + ".lengths"), int(m.group(3)),
            int(m.group(4)))


def table_of(path):
    lengths, starts, strands, row_block = mumsio.read_mums(path, with_blocks=True)
    return lengths, starts, strands, None if row_block is None else blocks_of_rows(row_block)


def test_fixture_set():
    """the conditions the fixtures were chosen for, checked on the fixtures themselves"""
    assert len(BEDS) == 8 * 6 + 6 + 8
    tables = {b: table_of(recorded(b)[0]) for b in BEDS}
    ends_in_block = {b for b, t in tables.items() if M.ends_in_block(t[3], len(t[0]))}
    ends_free = {b for b, t in tables.items() if t[3] is not None and not M.ends_in_block(t[3], len(t[0]))}
    assert any(b.startswith("minus_column.g1000") for b in ends_in_block) and ends_free
    assert all(t[3] is None or (t[3][:, 1] > t[3][:, 0]).all() for t in tables.values())            # no one-row block
    no_blocks = [b for b, t in tables.items() if t[3] is None]
    assert len(no_blocks) == 6 and all((tables[b][1] == -1).any() for b in no_blocks)
    for b in BEDS:                                           # -s 0, 1 and the last column, -L 100 and 0
        path, _, s, L = recorded(b)
        assert s in (0, 1, tables[b][1].shape[1] - 1) + ((3,) if b.startswith("inversion") else (2,)) and L in (0, 100)
    counts = {name: {len(x) for x in mumsio.read_contigs(os.path.join(GOLD, name + ".lengths"))[1]}
              for name in ("synteny", "inversion", "moved")}
    assert counts == {"synteny": {1}, "inversion": {3}, "moved": {40}}
    names, lens = mumsio.read_contigs(os.path.join(GOLD, "minus_column.lengths"))
    t = table_of(os.path.join(GOLD, "minus_column.g1000.mums"))
    for c, seq in enumerate(lens):
        assert seq[0] == 0 and 0 in seq[2:-1]
        begin = M.intervals(*t[:3], c, 0, t[3])[0]
        assert set(np.cumsum(seq).tolist()) & set(begin.tolist()), c       # a record begins exactly on a boundary
    minus = [open(os.path.join(GOLD, b)).read() for b in BEDS if b.startswith("minus_column.g1000.s2")]
    assert any("\t-\n" in x and "block_" in x for x in minus)              # blocks on '-'


@pytest.mark.parametrize("bed", BEDS, ids=[b[:-4] for b in BEDS])
def test_model_equals_the_reference_file(bed):
    path, lens_path, s, L = recorded(bed)
    lengths, starts, strands, blocks = table_of(path)
    contigs = mumsio.read_contigs(lens_path)
    want = open(os.path.join(GOLD, bed), "rb").read()
    open_tail = M.ends_in_block(blocks, len(lengths))
    assert M.bed_bytes(lengths, starts, strands, s, contigs, L, blocks, drop_open_tail=open_tail) == want
    ours = M.bed_bytes(lengths, starts, strands, s, contigs, L, blocks)
    if open_tail:                                            # departure 1: the block that ends the table is written
        extra = ours.replace(want, b"", 1) if want else ours
        assert ours.count(b"\n") == want.count(b"\n") + 1 and extra.count(b"\n") == 1
        assert b"\tblock_%d\t" % (len(blocks) - 1) in extra and b"\tblock_%d\t" % (len(blocks) - 1) not in want
    else:
        assert ours == want


# ---- the closed form, record by record ------------------------------------------------------------------------------------
def loop_bed(lengths, starts, strands, col, names, lens, L, blocks):
    """one record at a time, from the closed form; -> (lines, clamped)"""
    n = len(lengths)
    block_of = {}
    for b, (lo, hi) in enumerate([] if blocks is None else np.asarray(blocks).tolist()):
        for r in range(lo, hi + 1):
            block_of[r] = b
    out, clamped, i = [], 0, 0
    for r in range(n):
        start = int(starts[r][col])
        here = start != -1
        rec = None
        if blocks is not None:
            b = block_of.get(r)
            if b is not None and int(blocks[b][0]) == r:
                first, last = r, int(blocks[b][1])
                plus = bool(strands[last][col])
                if plus:
                    rec = (int(starts[first][col]), int(starts[last][col]) + int(lengths[last]), "block_%d" % b, plus)
                else:
                    rec = (int(starts[last][col]), int(starts[first][col]) + int(lengths[first]), "block_%d" % b, plus)
            elif b is None and int(lengths[r]) >= L:
                rec = (start, start + int(lengths[r]), "mum_%d" % i, bool(strands[r][col]))
        elif here and int(lengths[r]) >= L:
            rec = (start, start + int(lengths[r]), "mum_%d" % i, bool(strands[r][col]))
        i += here
        if rec is None:
            continue
        begin, end, label, plus = rec
        total, k = 0, None
        for j, v in enumerate(lens):
            total += v
            if total > begin:
                k, left = j, total - v
                break
        if k is None:
            k, left, clamped = len(lens) - 1, sum(lens) - lens[-1], clamped + 1
        out.append("%s\t%d\t%d\t%s\t%s\n" % (names[k], begin - left, begin - left + end - begin, label, "+" if plus else "-"))
    return "".join(out).encode(), clamped


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_plain_loop_with_blocks(seed):
    n = 150 + 17 * seed
    lengths, starts, strands, totals = M.make_rows(seed, n, 3)
    blocks = M.make_blocks(100 + seed, n)
    assert (blocks[:, 0] == blocks[:, 1]).any() and (blocks[:, 0] < blocks[:, 1]).any()
    contigs = M.make_contigs(200 + seed, [t - 4000 for t in totals], [1, 7, 40], zero=0.3)   # (short: some records are clamped)
    seen = 0
    for c in range(3):
        for L in (0, 100, 250):
            rec, clamped = M.records_of(lengths, starts, strands, c, contigs[1][c], L, blocks)
            want, want_clamped = loop_bed(lengths, starts, strands, c, contigs[0][c], contigs[1][c], L, blocks)
            assert M.text(rec, contigs[0][c]) == want and clamped == want_clamped
            seen += clamped
    assert seen


@pytest.mark.parametrize("seed", range(4))
def test_model_equals_the_plain_loop_with_partial_rows(seed):
    lengths, starts, strands, totals = M.make_rows(10 + seed, 200, 4, absent=0.3)
    contigs = M.make_contigs(300 + seed, totals, [1, 2, 5, 60], zero=0.2)
    for c in range(4):
        for L in (0, 150):
            rec, clamped = M.records_of(lengths, starts, strands, c, contigs[1][c], L)
            want, _ = loop_bed(lengths, starts, strands, c, contigs[0][c], contigs[1][c], L, None)
            assert M.text(rec, contigs[0][c]) == want and clamped == 0
            assert (rec[:, 3] < 0).all() and len(set(rec[:, 3].tolist())) == len(rec)
    rec, _ = M.records_of(lengths, starts, strands, 2, contigs[1][2], 0)
    assert (-1 - rec[:, 3]).tolist() == list(range(int((starts[:, 2] != -1).sum())))          # the rank, not the row
    assert len(rec) < len(lengths)


def test_model_edges():
    one = (np.array([50], np.uint32), np.array([[10, 99]], np.int64), np.array([[True, False]]))
    lens = [0, 10, 0, 90, 100]
    rec, cl = M.records_of(*one, 0, lens, 0)                 # begin exactly on the boundary behind c1: c3, never the empty z2
    assert rec.tolist() == [[3, 0, 50, -1, 1]] and cl == 0
    rec, cl = M.records_of(*one, 1, lens, 0)
    assert rec.tolist() == [[3, 89, 139, -1, 0]] and cl == 0    # runs over the end of c3: not split
    rec, cl = M.records_of(*one, 1, [5, 94, 0], 0)           # begin == the total: the last contig, counted
    assert rec.tolist() == [[2, 0, 50, -1, 0]] and cl == 1
    assert M.text(rec, ["p", "q", "r"]) == b"r\t0\t50\tmum_0\t-\n"
    rec, _ = M.records_of(*one, 0, lens, 51)
    assert len(rec) == 0
    rec, _ = M.records_of(*one, 0, lens, 51, blocks=np.array([[0, 0]]))                      # departure 2: a one-row block
    assert rec.tolist() == [[3, 0, 50, 0, 1]]


# ---- the reader of the contig table ---------------------------------------------------------------------------------------
def test_read_contigs(tmp_path):
    for name in ("synteny", "inversion", "moved", "minus_column", "partial"):
        path = os.path.join(GOLD, name + ".lengths")
        names, lens = mumsio.read_contigs(path)
        lines = [l.split() for l in open(path).read().splitlines()]
        assert [n for seq in names for n in seq] == [l[1] for l in lines if l[1] != "*"]
        assert [v for seq in lens for v in seq] == [int(l[2]) for l in lines if l[1] != "*"]
        assert len(names) == len(lens) == sum(l[1] == "*" for l in lines)
        assert [sum(x) for x in lens] == mumsio.read_seq_lengths(path) == [int(l[2]) for l in lines if l[1] == "*"]
    plain = tmp_path / "plain.lengths"
    plain.write_text("/a.fa 100\n/b.fa 200\n")
    with pytest.raises(ValueError, match="multi-FASTA-aware run"):
        mumsio.read_contigs(str(plain))


def test_contig_tables():
    begin, lens, name_begin, blob = binding.contig_tables(([["a", "bcd"], [], ["ef"]], [[5, 0], [], [7]]))
    assert begin.tolist() == [0, 2, 2, 3] and lens.tolist()[:3] == [5, 0, 7] and name_begin.tolist() == [0, 1, 4, 6]
    assert blob == b"abcdef" and begin.dtype == np.uint64 and lens.dtype == np.int64 and name_begin.dtype == np.uint64
    with pytest.raises(binding.MumemtoError, match="tab or a newline"):
        binding.contig_tables(([["a\tb"]], [[5]]))
    with pytest.raises(binding.MumemtoError, match="do not match"):
        binding.contig_tables(([["a"]], [[5, 6]]))


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_and_documented():
    header = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    api = open(os.path.join(ROOT, "mumemto_amd", "csrc", "api.cpp")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"MMT_API [\w\s\*]+\b%s\(" % name, header), name
        assert re.search(r"\b%s\(" % name, api), name
        assert name in binding.GPU_ABI_SYMBOLS, name
    assert "mumemto/mum_to_bed.py" in header
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "mum_to_bed" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "The BED writer is in" in design
    import mumemto_amd
    assert callable(mumemto_amd.mum_to_bed) and "mum_to_bed" in dir(mumemto_amd)
    for method in ("bed", "bed_records", "bed_records_device", "bed_text", "write_bed", "bed_stats"):
        assert callable(getattr(mumemto_amd.Merged, method)), method


def test_build_lists_the_sources():
    from mumemto_amd import build
    assert "bed.cpp" in build.LIB_SOURCES and "bed_kernels.hip" in build.LIB_SOURCES
    for f in ("bed.cpp", "bed.hpp", "bed_kernels.hip", "bed_kernels.hpp"):
        assert os.path.exists(os.path.join(ROOT, "mumemto_amd", "csrc", f)), f
    consts = open(os.path.join(ROOT, "mumemto_amd", "csrc", "bed_kernels.hpp")).read()
    for name in ("SELECT_BLOCK", "SELECT_ITEMS", "BED_LDS_CONTIGS", "BED_WAVE_RECORDS", "BED_LDS_BYTES"):
        assert re.search(r"%s\s*=\s*\d+" % name, consts), name


def test_tool_arguments(tmp_path):
    from mumemto_amd.mum_to_bed import parse_arguments
    r = subprocess.run(TOOL + ["--help"], cwd=ROOT, capture_output=True, timeout=120)      # (argparse leaves before the library loads)
    assert r.returncode == 0 and b"--min-singleton-length" in r.stdout and b"--all" in r.stdout
    a = parse_arguments(["x/run.mums"])
    assert (a.lengths_file, a.seq_idx, a.min_singleton_length, a.output, a.verbose, a.all, a.max_block_gap) == \
        (os.path.join("x", "run.lengths"), 0, 100, None, False, False, None)
    a = parse_arguments(["run.bumbl", "-l", "other.lengths", "-s", "3", "-L", "0", "-o", "out.bed", "-v", "-g", "500"])
    assert (a.lengths_file, a.seq_idx, a.min_singleton_length, a.output, a.verbose, a.max_block_gap) == \
        ("other.lengths", 3, 0, "out.bed", True, 500)
    a = parse_arguments(["run.mums", "--all", "-o", "prefix"])
    assert a.all and a.output == "prefix"
    r = subprocess.run(TOOL + ["run.mums", "--all"], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 2 and b"--all needs -o" in r.stderr
    with pytest.raises(SystemExit):
        parse_arguments(["run.mums", "--all", "-s", "1", "-o", "p"])


def test_tool_refuses_before_the_library_is_needed(tmp_path):
    plain = tmp_path / "t.lengths"
    plain.write_text("/a.fa 100\n")
    mums = tmp_path / "t.mums"
    mums.write_text("30\t5\t+\n")
    r = subprocess.run(TOOL + [str(mums)], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"multi-FASTA-aware run" in r.stderr and r.stdout == b""
    r = subprocess.run(TOOL + [os.path.join(GOLD, "synteny.g1000.mums"), "-l", os.path.join(GOLD, "synteny.lengths"), "-s", "3"],
                       cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Sequence index 3 too large for dataset with 3 sequences." in r.stderr
    r = subprocess.run(TOOL + [str(tmp_path / "t.txt"), "-l", os.path.join(GOLD, "synteny.lengths")], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 1 and b"does not end with .mums or .bumbl" in r.stderr
