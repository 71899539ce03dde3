"""OutFile (mumemto_amd/csrc/out_file.hpp), the one output file behind every writer of the library: a stand-alone program
(tests/out_file_check.cpp) under the host sanitizers writes 10,001 bytes in pieces of 1, 4095 and 4097 bytes and checks what
commit, abort, an IN_PLACE abort, a failed write and the early removal of an earlier run's file (retire_old) leave behind.
Host only."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mumemto_amd", "csrc")


def test_out_file_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "out_file_check")
    # (the sanitizers' runtimes inside the program: it runs as it is, whatever the environment preloads)
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "out_file_check.cpp"), "-o", exe], check=True)
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "out_file ok"
    assert os.listdir(work) == []
