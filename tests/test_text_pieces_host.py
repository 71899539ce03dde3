"""Host: where a text of whole lines is cut into pieces (cut_pieces, mumemto_amd/csrc/piece_cut.hpp -- the rule of
write_merged_text, label_write_text and bed_write_text), as a stand-alone program under the host sanitizers
(tests/piece_cut_check.cpp), against the model below: a piece takes whole lines while they fit the limit, and a line longer
than the limit is a piece of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mumemto_amd", "csrc")


def model(lengths, piece):
    cut, longest, size = [0], 0, 0
    for r, n in enumerate(lengths):
        if r > cut[-1] and size + n > piece:           # the line does not fit behind the others: they are a piece
            cut.append(r)
            longest, size = max(longest, size), 0
        size += n
    if lengths:
        cut.append(len(lengths))
        longest = max(longest, size)
    return cut, longest


CASES = {
    "zero lines": ([], 100),
    "everything in one piece": ([30, 30, 30], 100),
    "a piece that ends exactly on the limit": ([40, 60, 50, 50, 10], 100),
    "a piece that ends one byte over the limit": ([40, 61, 50, 50, 10], 100),
    "a long line between short lines": ([10, 20, 250, 20, 10], 100),
    "a long line first": ([250, 20, 10, 80], 100),
    "a long line last": ([10, 20, 80, 250], 100),
    "a long line alone": ([250], 100),
    "every line on the limit": ([100, 100, 100], 100),
    "random": (np.random.default_rng(7).integers(1, 301, 1000).tolist(), 4096),
}


@pytest.fixture(scope="module")
def cuts(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("piece_cut")
    exe = str(d / "piece_cut_check")
    # (the sanitizers' runtimes inside the program: it runs as it is, whatever the environment preloads)
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "piece_cut_check.cpp"), "-o", exe], check=True)
    path = d / "cases.txt"
    path.write_text("".join("%d %d %s\n" % (piece, len(lengths), " ".join(map(str, np.cumsum([0] + lengths).tolist())))
                            for lengths, piece in CASES.values()))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [list(map(int, l.split())) for l in r.stdout.splitlines()]
    assert len(out) == len(CASES)
    return {name: (row[1:], row[0]) for name, row in zip(CASES, out)}


@pytest.mark.parametrize("name", list(CASES))
def test_cuts_against_the_model(cuts, name):
    lengths, piece = CASES[name]
    cut, longest = cuts[name]
    assert (cut, longest) == model(lengths, piece)
    # the cuts cover [0, n] without gaps, and a piece is at most the limit unless it is a single line
    assert cut[0] == 0 and cut[-1] == len(lengths) and all(a < b for a, b in zip(cut, cut[1:]))
    sizes = [sum(lengths[a:b]) for a, b in zip(cut, cut[1:])]
    assert all(s <= piece or b == a + 1 for s, a, b in zip(sizes, cut, cut[1:]))
    assert longest == max(sizes, default=0)
    # and no piece could have taken the line behind it
    assert all(s + lengths[b] > piece for s, b in zip(sizes[:-1], cut[1:-1]))


def test_the_cases_are_the_ones_meant():
    assert model(*CASES["a piece that ends exactly on the limit"])[0] == [0, 2, 4, 5]
    assert model(*CASES["a piece that ends one byte over the limit"])[0] == [0, 1, 2, 4, 5]
    assert model(*CASES["a long line between short lines"])[0] == [0, 2, 3, 5]
    assert model(*CASES["a long line first"])[0] == [0, 1, 3, 4] and model(*CASES["a long line last"])[0] == [0, 2, 3, 4]
    assert len(model(*CASES["random"])[0]) > 30
