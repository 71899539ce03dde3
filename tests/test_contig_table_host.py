"""Host: the one check of the contig tables (mumemto_amd/csrc/contig_table.cpp) that bed() and label() share, as a
stand-alone program under the host sanitizers (tests/contig_table_check.cpp).  Every refusal is held to the message bed.cpp
and label.cpp threw before they shared the check -- the literals below are copied from those sources --, a fault in a column
bed() was not asked for goes unreported, and the ends and totals of a table with empty contigs are summed here again."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mumemto_amd", "csrc")

# three sequences of 2, 1 and 3 contigs
NAMES = [["a0", "a1"], ["b0"], ["c0", "c1", "c2"]]
LENS = [[10, 0], [7], [0, 5, 0]]


def tables(names=NAMES, lens=LENS):
    begin, length, name_begin, blob = [0], [], [0], b""
    for seq_names, seq_lens in zip(names, lens):
        begin.append(begin[-1] + len(seq_lens))
        length += seq_lens
        for name in seq_names:
            blob += name.encode()
            name_begin.append(len(blob))
    return dict(begin=begin, len=length, name_begin=name_begin, names=blob)


def line(who, t, first=0, last=None, use_names=1, **replace):
    t = dict(t, **replace)
    field = lambda v: "-" if v is None else ",".join(map(str, v))      # noqa: E731
    n_docs = len(t["begin"]) - 1 if t["begin"] is not None else 3
    return ";".join([who, str(first), str(n_docs if last is None else last), str(n_docs), str(use_names), field(t["begin"]),
                     field(t["len"]), field(t["name_begin"]), "-" if t["names"] is None else t["names"].hex(), "end"])


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("contig_table")
    exe = str(d / "contig_table_check")
    # (the sanitizers' runtimes inside the program: it runs as it is, whatever the environment preloads)
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "contig_table_check.cpp"), "-o", exe], check=True)

    def run_cases(lines):
        path = d / "cases.txt"
        path.write_text("".join(l + "\n" for l in lines))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run_cases


def with_lens(lens):
    return tables(lens=lens)


def with_name(seq, k, name):
    names = [list(x) for x in NAMES]
    names[seq][k] = name
    return tables(names=names)


T = tables()
NO_SEQ_1 = tables(names=[NAMES[0], [], NAMES[2]], lens=[LENS[0], [], LENS[2]])
# (who, the case, the message of the parent's bed.cpp / label.cpp)
REFUSALS = [
    ("bed", line("bed", T, begin=None), "bed: contig_begin must hold n_docs + 1 entries"),
    ("label", line("label", T, begin=None), "label: contig_begin must hold n_docs + 1 entries"),
    ("bed", line("bed", T, begin=[0, 3, 2, 6]), "bed: contig_begin does not ascend"),
    ("label", line("label", T, begin=[0, 3, 2, 6]), "label: contig_begin does not ascend"),
    ("bed", line("bed", T, len=None), "bed: contig_len and name_begin must hold an entry per contig (name_begin one more)"),
    ("bed", line("bed", T, name_begin=None), "bed: contig_len and name_begin must hold an entry per contig (name_begin one more)"),
    ("label", line("label", T, len=None), "label: contig_len must hold an entry per contig"),
    ("label", line("label", T, name_begin=None), "label: name_begin must hold an entry per contig and one more"),
    ("bed", line("bed", T, name_begin=[0, 2, 4, 3, 8, 10, 12]), "bed: name_begin does not ascend"),
    ("label", line("label", T, name_begin=[0, 2, 4, 3, 8, 10, 12]), "label: name_begin does not ascend"),
    ("bed", line("bed", T, names=None), "bed: names must hold the bytes name_begin refers to"),
    ("label", line("label", T, names=None), "label: names must hold the bytes name_begin refers to"),
    ("bed", line("bed", NO_SEQ_1), "bed: sequence 1 has no contigs"),
    ("label", line("label", NO_SEQ_1), "label: sequence 1 has no contigs"),
    ("bed", line("bed", with_lens([[10, 0], [7], [0, -5, 9]])), "bed: contig 1 of sequence 2 has the negative length -5"),
    ("label", line("label", with_lens([[10, 0], [7], [0, -5, 9]])), "label: contig 1 of sequence 2 has the negative length -5"),
    ("bed", line("bed", with_lens([[1 << 61, 1 << 61], [7], [0, 5, 0]])), "bed: sequence 0 is 2^62 bases or longer"),
    ("label", line("label", with_lens([[1 << 61, 1 << 61], [7], [0, 5, 0]])), "label: sequence 0 is 2^62 bases or longer"),
    ("bed", line("bed", with_lens([[10, 0], [0], [0, 5, 0]])), "bed: sequence 1 has total length 0: no contig can hold an interval"),
    ("label", line("label", with_lens([[10, 0], [0], [0, 5, 0]])), "label: sequence 1 has total length 0: no contig can hold a start"),
    ("bed", line("bed", with_name(1, 0, "b\t0")), "bed: the name of contig 0 of sequence 1 contains a tab or a newline"),
    ("bed", line("bed", with_name(2, 1, "c\n1")), "bed: the name of contig 1 of sequence 2 contains a tab or a newline"),
    ("label", line("label", with_name(1, 0, "b\t0")), "label: the name of contig 0 of sequence 1 contains a tab, a newline or a comma"),
    ("label", line("label", with_name(1, 0, "b\n0")), "label: the name of contig 0 of sequence 1 contains a tab, a newline or a comma"),
    ("label", line("label", with_name(2, 2, "c,2")), "label: the name of contig 2 of sequence 2 contains a tab, a newline or a comma"),
]


def test_every_refusal_keeps_its_message(run):
    out = run([case for _, case, _ in REFUSALS])
    for (who, case, want), got in zip(REFUSALS, out):
        assert got == "refused;" + want, case


def expected(t, first, last, use_names):
    ends, totals, longest = [], [], []
    for c in range(len(t["begin"]) - 1):
        run_ = 0
        names = []
        for g in range(t["begin"][c], t["begin"][c + 1]):
            run_ += t["len"][g]
            ends.append(run_)
            names.append(t["name_begin"][g + 1] - t["name_begin"][g])
        totals.append(run_)
        longest.append(max(names) if use_names and first <= c < last else 0)
    return "ok;%d;%d;%s;%s;%s" % (t["begin"][-1], len(t["names"]) if use_names else 0, ",".join(map(str, ends + [0])),
                                  ",".join(map(str, totals)), ",".join(map(str, longest)))


def test_what_is_allowed_and_the_sums(run):
    comma = with_name(1, 0, "b,0")                    # a comma is a fault only where names are listed with commas
    long_names = tables(names=[["a0", "a" * 300], ["b0"], ["c0", "c1", "c" * 70]])
    cases = [(line("bed", T), expected(T, 0, 3, True)),
             (line("label", T), expected(T, 0, 3, True)),
             (line("bed", comma), expected(comma, 0, 3, True)),
             (line("label", long_names), expected(long_names, 0, 3, True)),
             # label without names: neither name_begin nor names is looked at
             (line("label", with_name(1, 0, "b\t0"), use_names=0), expected(T, 0, 3, False)),
             (line("label", T, use_names=0, name_begin=None, names=None), expected(T, 0, 3, False))]
    # bed asked for column 0 alone: a fault in column 1 or 2 is not reported
    for faulty in (NO_SEQ_1, with_lens([[10, 0], [7], [0, -5, 9]]), with_lens([[10, 0], [0], [0, 5, 0]]), with_name(1, 0, "b\t0"),
                   with_lens([[10, 0], [7], [1 << 61, 1 << 61, 0]])):
        cases.append((line("bed", faulty, first=0, last=1), expected(faulty, 0, 1, True)))
    out = run([c for c, _ in cases])
    for (case, want), got in zip(cases, out):
        assert got == want, case
    # and the same faults are reported once their column is asked for
    assert run([line("bed", NO_SEQ_1, first=1, last=2)]) == ["refused;bed: sequence 1 has no contigs"]
    assert run([line("bed", with_name(1, 0, "b\t0"), first=1, last=2)]) == [
        "refused;bed: the name of contig 0 of sequence 1 contains a tab or a newline"]
    assert run([line("bed", with_name(1, 0, "b\t0"), first=2, last=3)])[0].startswith("ok;")
