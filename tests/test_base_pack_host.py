"""pack_bases (mumemto_amd/csrc/base_pack.cpp), the host half of the two-bit transport of FASTA chunks: a stand-alone
program (tests/base_pack_check.cpp) under the host sanitizers holds the AVX2 and the scalar body to a byte loop on every
length 0..130, 4095..4097 and 1,048,583, every content class, three source misalignments, guard words behind both outputs
and the run cap.  The numpy model the GPU test uses (tests/basepack_model.py) is held to the same byte loop here, so a
broken model cannot pass there vacuously.  Host only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import basepack_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mumemto_amd", "csrc")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("base_pack") / "base_pack_check")
    # (the sanitizers' runtimes inside the program: it runs as it is, whatever the environment preloads)
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "base_pack_check.cpp"), "-o", exe], check=True)
    return exe


def test_both_bodies_against_the_byte_loop_under_the_host_sanitizers(check_exe):
    for env in (dict(os.environ), dict(os.environ, MUMEMTO_NO_AVX2="1")):      # (pack_bases itself: either body)
        r = subprocess.run([check_exe], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.strip() == "base_pack ok"


def byte_loop(check_exe, tmp_path, bases):
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(bases.tobytes())
    subprocess.run([check_exe, "pack", str(src), str(out)], check=True)
    raw = out.read_bytes()
    n_words, n_runs = np.frombuffer(raw[:16], np.uint64)
    words = np.frombuffer(raw[16:16 + 8 * int(n_words)], np.uint64)
    runs = np.frombuffer(raw[16 + 8 * int(n_words):], np.uint32).reshape(-1, 3)
    assert len(runs) == n_runs
    return words, runs


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 130, 4097, 70001])
def test_the_numpy_model_against_the_byte_loop(check_exe, tmp_path, n):
    fold = np.arange(256, dtype=np.uint8)
    for lower, upper in zip(b"acgt", b"ACGT"):
        fold[lower] = upper                                # (what comes back: a c g t as A C G T, every other byte verbatim)
    for name, bases in M.contents(n).items():
        want_words, want_runs = byte_loop(check_exe, tmp_path, bases)
        words, runs = M.pack(bases)
        assert np.array_equal(words, want_words), name
        assert np.array_equal(runs, want_runs), name
        assert np.array_equal(M.unpack(want_words, n, want_runs), fold[bases]), name
