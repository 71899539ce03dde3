"""Host: the model of the multi-MUM sequence writer (tests/seqmodel.py) against the files the reference's own extract_mums
binary wrote (tests/golden/string_merge/*/p*_mums.fa, with their .mums, .lengths and FASTA files), and the surface of the
feature: header, exports, binding, the tool's argument handling.  Every comparison is exact.

The PYTHON dialect cannot be recorded: the reference's Python tool needs Biopython, which is not available.  It is held to
expectations written by hand in this file, for a dozen rows on one short sequence."""
import glob
import os
import re
import subprocess
import sys

import pytest

import seqmodel as M
from mumemto_amd import binding, mumsio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "string_merge")
PARTS = sorted(p[: -len("_mums.fa")] for p in glob.glob(os.path.join(GOLD, "*", "p*_mums.fa")))
ENTRY_POINTS = ("mmt_merged_sequences", "mmt_merged_sequences_host", "mmt_merged_sequences_file", "mmt_merged_sequences_offsets",
                "mmt_merged_sequences_offsets_device", "mmt_merged_sequences_text", "mmt_merged_sequences_write_text",
                "mmt_merged_sequences_stats")
TOOL = [sys.executable, "-m", "mumemto_amd.extract_mums"]


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_document(prefix):
    """the bases of the first document PREFIX.lengths names (paths relative to the fixture's directory)"""
    name = read(prefix + ".lengths").split()[0].decode()
    return M.read_fasta(os.path.join(os.path.dirname(prefix), name))


def test_fixture_set():
    assert len(PARTS) == 9 and len({os.path.dirname(p) for p in PARTS}) == 4


@pytest.mark.parametrize("prefix", PARTS, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_binary_dialect_reproduces_the_reference_binary(prefix):
    lengths, starts, strands = mumsio.read_mums(prefix + ".mums")
    seq, want = first_document(prefix), read(prefix + "_mums.fa")
    assert len(lengths) > 0 and want.count(b">mum_") == len(lengths)
    assert M.sequences(seq, lengths, starts, strands, 0, M.BINARY, True) == want
    # -t: the same records without the `#` (no base is a `#`)
    assert want.count(b"#") == len(lengths)
    assert M.sequences(seq, lengths, starts, strands, 0, M.BINARY, False) == want.replace(b"#\n", b"\n")
    # the counts, from the recorded file itself: every line behind a header holds the record's bases and the `#`
    recorded = [len(l) - 1 for l in want.split(b"\n")[1::2]]
    records, bases, clipped, empty = M.stats(seq, lengths, starts, 0, M.BINARY)
    assert (records, bases, empty) == (len(lengths), sum(recorded), recorded.count(0))
    assert clipped == sum(r < int(l) for r, l in zip(recorded, lengths))


#            0         1         2         3
#            0123456789012345678901234567890123456789
SEQ = b"ACGTacgtNNRYKMSWBDHVXnAAACCCGGGTTTacgtAC"         # 40 bases: lower case, N, every IUPAC code, X
ROWS = [  # (length, start, '+'), the bases PYTHON gives, the bases BINARY gives (None: refused)
    ((4, 0, True), b"ACGT", b"ACGT"),
    ((4, 0, False), b"ACGT", b"ACGT"),                      # its own reverse complement
    ((6, 2, True), b"GTACGT", b"GTacgt"),                   # lower case: upper-cased by PYTHON alone
    ((6, 2, False), b"ACGTAC", b"GTacgt"),
    ((5, 6, True), b"GTNNR", b"gtNNR"),                     # N and an IUPAC code
    ((5, 6, False), b"YNNAC", b"gtNNR"),                    # R -> Y, N stays
    ((12, 10, False), b"NXBDHVWSKMRY", b"RYKMSWBDHVXn"),    # every pair of the table; W, S, X, N stay
    ((10, 22, True), b"AAACCCGGGT", b"AAACCCGGGT"),
    ((10, 22, False), b"ACCCGGGTTT", b"AAACCCGGGT"),
    ((9, 36, True), b"GTAC", b"gtAC"),                      # runs over the end: cut there
    ((9, 36, False), b"GTAC", b"gtAC"),
    ((5, 40, True), b"", b""),                              # starts exactly at the end: empty
    ((5, 41, True), b"", None),                             # starts beyond the end
    ((5, -1, False), b"", None),                            # no start in this sequence (partial)
    ((0, 3, True), b"", b""),                               # a row of no bases
]


def table(rows):
    lengths = [r[0] for r in rows]
    return lengths, [[7, r[1]] for r in rows], [[True, r[2]] for r in rows]     # the sequence is column 1 of two


def test_python_dialect_hand_written_rows():
    """hand-written: both strands, lower case, N and IUPAC codes, the clipped row, the empty row, the partial row"""
    lengths, starts, strands = table([r for r, _, _ in ROWS])
    for term in (True, False):
        t = b"#" if term else b""
        want = b"\n".join(b">mum_%d\n" % i + py + t for i, (_, py, _) in enumerate(ROWS))
        assert M.sequences(SEQ, lengths, starts, strands, 1, M.PYTHON, term) == want
        assert want.endswith(b">mum_14\n" + t) and want.count(b">mum_") == len(ROWS)     # no newline behind the last record
    # cut at the end: the two rows from 36 and the one from 40; empty: from 40, from 41, the partial row, the row of no bases
    assert M.stats(SEQ, lengths, starts, 1) == (15, sum(len(py) for _, py, _ in ROWS), 3, 4)
    assert M.sequences(SEQ, [], [], [], 0, M.PYTHON) == b"" == M.sequences(SEQ, [], [], [], 0, M.BINARY)


def test_binary_dialect_hand_written_rows():
    kept = [(r, b) for r, _, b in ROWS if b is not None]
    lengths, starts, strands = table([r for r, _ in kept])
    assert M.sequences(SEQ, lengths, starts, strands, 1, M.BINARY) == b"".join(b">mum_%d\n%s#\n" % (i, b) for i, (_, b) in enumerate(kept))
    assert M.sequences(SEQ, lengths, starts, strands, 1, M.BINARY, False) == b"".join(b">mum_%d\n%s\n" % (i, b) for i, (_, b) in enumerate(kept))


def test_refusals_of_the_model():
    lengths, starts, strands = table([r for r, _, _ in ROWS])
    for col in (-1, 2):
        with pytest.raises(M.Refused) as ex:
            M.sequences(SEQ, lengths, starts, strands, col)
        assert ex.value.kind == "column"
    with pytest.raises(M.Refused) as ex:
        M.sequences(SEQ, lengths, starts, strands, 1, M.BINARY)
    assert (ex.value.kind, ex.value.row) == ("partial", 13)
    with pytest.raises(M.Refused) as ex:
        M.sequences(SEQ, lengths[:13], starts[:13], strands[:13], 1, M.BINARY)
    assert (ex.value.kind, ex.value.row) == ("beyond", 12)
    for dialect in (M.BINARY, M.PYTHON):
        with pytest.raises(M.Refused) as ex:
            M.sequences(SEQ, [3, 3], [[0, 1], [0, -2]], [[True, True]] * 2, 1, dialect)
        assert (ex.value.kind, ex.value.row) == ("start", 1)


def test_complement_table():
    pairs = "AT CG MK RY VB HD"
    for a, b in pairs.split():
        assert M.reverse_complement(a.encode()) == b.encode() and M.reverse_complement(b.encode()) == a.encode()
    others = bytes(c for c in range(256) if chr(c) not in pairs)
    assert M.reverse_complement(others) == others[::-1]


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_header_sources_and_exports():
    header = read(os.path.join(ROOT, "include", "mumemto_gpu.h")).decode()
    api = read(os.path.join(ROOT, "mumemto_amd", "csrc", "api.cpp")).decode()
    for name in ENTRY_POINTS + ("mmt_engine_text_packed",):
        assert re.search(r"MMT_API [\w\s\*]+\b%s\(" % name, header), name
        assert re.search(r"\b%s\(" % name, api), name
    assert "mmt_seq_binary = 0, mmt_seq_python = 1" in header
    build = read(os.path.join(ROOT, "mumemto_amd", "build.py")).decode()
    assert '"sequences.cpp"' in build and '"sequence_kernels.hip"' in build
    import mumemto_amd
    assert callable(mumemto_amd.extract_mums) and mumemto_amd.extract_mums is binding.extract_mums
    for name in ("sequences", "sequences_text", "write_sequences", "sequences_stats", "sequences_offsets"):
        assert callable(getattr(binding.Merged, name)), name
    assert callable(binding.Engine.mum_sequences)
    assert binding.SEQ_DIALECTS == {"binary": 0, "python": 1}


def test_the_module_stays_callable():
    import mumemto_amd.extract_mums as tool
    assert callable(tool) and callable(tool.main) and callable(tool.parse_arguments)


def test_tool_help_works_without_the_library():
    r = subprocess.run(TOOL + ["--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)     # (argparse leaves before the library loads)
    assert r.returncode == 0
    for flag in ("-m", "--mumfile", "-i", "--index", "-o", "--output", "-f", "--filelist", "-v", "--verbose", "-t",
                 "--no-terminator", "--dialect", "--device"):
        assert flag in r.stdout, flag


def test_tool_default_names(tmp_path):
    from mumemto_amd import extract_mums as tool_module
    (tmp_path / "run.lengths").write_text("a.fa 10\n")
    stem = str(tmp_path / "run")
    a = tool_module.parse_arguments(["-m", stem + ".mums"])
    assert (a.index, a.output, a.filelist, a.dialect, a.terminator, a.verbose) == (0, stem + "_mums.fa", stem + ".lengths", "python", True, False)
    assert tool_module.parse_arguments(["-m", stem + ".bumbl", "-o", "x"]).output == "x.fa"
    assert tool_module.parse_arguments(["-m", stem + ".mums", "-o", "x.fa"]).output == "x.fa"
    assert tool_module.parse_arguments(["-m", stem + ".mums", "-o", "x.fasta"]).output == "x.fasta"
    assert tool_module.parse_arguments(["-m", stem + ".mums", "-o", "x.txt"]).output == "x.txt.fa"
    a = tool_module.parse_arguments(["-m", stem + ".mums", "-f", "other.lengths", "-i", "3", "-t", "--dialect", "binary", "-v"])
    assert (a.filelist, a.index, a.terminator, a.dialect, a.verbose) == ("other.lengths", 3, False, "binary", True)
    # the FASTA path of sequence i: the first token of line i, or of the i-th `*` line of a multi-FASTA lengths file
    (tmp_path / "multi.lengths").write_text("a.fa * 10\na.fa r0 4\na.fa r1 6\nb.fa * 5\nb.fa r0 5\n")
    assert tool_module.seq_paths(str(tmp_path / "multi.lengths")) == ["a.fa", "b.fa"]
    (tmp_path / "plain.lengths").write_text("a.fa 10\nb.fa 5\n")
    assert tool_module.seq_paths(str(tmp_path / "plain.lengths")) == ["a.fa", "b.fa"]


def test_tool_refusals_before_the_library_loads(tmp_path):
    """each ends with exit 1 (2 from argparse) and its message, and leaves no output file behind"""
    stem = str(tmp_path / "run")
    doc = str(tmp_path / "doc.fa")
    (tmp_path / "doc.fa").write_text(">r\nACGTACGTAC\n")
    (tmp_path / "run.mums").write_text("4\t0,1\t+,+\n")

    def run(args):
        r = subprocess.run(TOOL + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith((".tmp", "_mums.fa"))] and r.stdout == ""
        return r.returncode, r.stderr

    rc, err = run(["-m", stem + ".mums"])                                      # no filelist beside the table
    assert rc == 1 and "Filelist %s.lengths not found, and no filelist provided" % stem in err
    assert run([])[0] == 2                                                     # -m is required
    assert run(["-m", stem + ".mums", "--dialect", "perl"])[0] == 2
    (tmp_path / "run.lengths").write_text("%s 10\n/nowhere/gone.fa 10\n" % doc)
    rc, err = run(["-m", stem + ".mums", "-i", "2"])
    assert rc == 1 and "index 2 is out of range" in err
    rc, err = run(["-m", stem + ".mums", "-i", "-1"])
    assert rc == 1 and "index -1 is out of range" in err
    rc, err = run(["-m", stem + ".mums", "-i", "1"])
    assert rc == 1 and "File /nowhere/gone.fa not found" in err and "Perhaps the paths are relative, not absolute?" in err
    rc, err = run(["-m", str(tmp_path / "absent.mums"), "-f", stem + ".lengths"])
    assert rc == 1 and "absent.mums" in err
    (tmp_path / "run.lengths").write_text("%s 10\n" % doc)
    rc, err = run(["-m", stem + ".mums"])                                      # a table of two sequences, a list of one
    assert rc == 1 and "has 2 sequences" in err and "lists 1" in err
    (tmp_path / "run.lengths").write_text("%s\n" % doc)
    rc, err = run(["-m", stem + ".mums"])                                      # a lengths file without lengths
    assert rc == 1 and "cannot read the filelist" in err


def test_merge_driver_flag():
    from mumemto_amd import merge_mums
    a = merge_mums.parse_arguments(["a.mums", "b.mums"])
    assert a.extract_on_device is False
    assert merge_mums.parse_arguments(["a.mums", "b.mums", "--extract-on-device"]).extract_on_device is True
