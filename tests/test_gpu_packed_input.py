"""The two-bit transport of FASTA chunks on the device: k::unpack_bases through its probe (tests/kprobe_input/kprobe_input.cpp
kpi_unpack_bases) against the numpy model of tests/basepack_model.py -- which tests/test_base_pack_host.py holds to the
packer's byte loop --, and mumemto_exec's one-shot path end to end: packed (either packer body) and unpacked input must
leave the same files, byte for byte.  All comparisons are exact."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import basepack_model as M
from mumemto_amd import build

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(build.LIB), "..", "bin", "mumemto_exec")
PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kprobe_input", "libkprobe_input.so")
SENT8 = 0xA5
GUARD = 64                      # sentinel bytes in front of the destination and behind it
OFFSETS = (0, 1, 7, 15)         # the destination's distance from a 16-byte boundary
SIZES = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, (1 << 20) + 7]


def probe():
    lib = ctypes.CDLL(PROBE)
    lib.kpi_last_error.restype = ctypes.c_char_p
    return lib


def unpack_on_device(words, n, runs, off):
    """(the n bytes written, the bytes in front, the bytes behind) with the destination `off` bytes behind a 16-byte boundary"""
    buf = np.full(GUARD + off + n + GUARD, SENT8, np.uint8)
    runs = np.ascontiguousarray(runs, np.uint32).reshape(-1, 3)
    words = np.ascontiguousarray(words, np.uint64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib = probe()
    rc = lib.kpi_unpack_bases(ptr(words), len(words), n, ptr(runs), len(runs), ptr(buf), len(buf), GUARD + off)
    assert rc == 0, lib.kpi_last_error().decode()
    return buf[GUARD + off:GUARD + off + n], buf[:GUARD + off], buf[GUARD + off + n:]


def check(bases, what):
    n = len(bases)
    words, runs = M.pack(bases)
    want = M.unpack(words, n, runs)
    for off in OFFSETS:
        got, front, behind = unpack_on_device(words, n, runs, off)
        assert np.array_equal(got, want), (what, n, off)
        assert (front == SENT8).all() and (behind == SENT8).all(), (what, n, off)


@pytest.mark.parametrize("n", SIZES)
def test_unpack_bases_every_content_class(n):
    for name, bases in M.contents(n).items():
        check(bases, name)


def test_unpack_bases_a_long_run_of_n():
    n = (1 << 20) + 7
    bases = M.contents(n)["ACGTacgt"]
    bases[400_003:700_003] = ord("N")
    bases[700_003:700_010] = ord("n")
    check(bases, "300,000 N")


# ---- end to end: mumemto_exec over four small files, chunks of 1 MB --------------------------------------------------
CHUNK = 1 << 20
BASES = 2_600_000


def write_fasta(path, name, bases, width=60):
    with open(path, "wb") as f:
        f.write(b">" + name + b"\n")
        whole = len(bases) // width * width
        lines = np.empty((whole // width, width + 1), np.uint8)
        lines[:, :width] = bases[:whole].reshape(-1, width)
        lines[:, width] = ord("\n")
        f.write(lines.tobytes())
        if whole < len(bases):
            f.write(bases[whole:].tobytes() + b"\n")


@pytest.fixture(scope="module")
def collection(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("packed_input")
    rng = np.random.default_rng(77)
    anchor = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, BASES)]

    def variant():
        v = anchor.copy()
        at = rng.integers(0, BASES, BASES // 500)
        v[at] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(at))]
        return v

    plain = variant()
    masked = variant()
    for at in rng.integers(0, BASES - 5000, 150):
        masked[at:at + int(rng.integers(1, 5000))] |= 0x20                     # stretches of lower case
    runs = variant()
    runs[1000] = ord("N")
    runs[5000:5050] = ord("N")
    runs[300_000:500_000] = ord("N")
    runs[CHUNK - 76:CHUNK + 124] = ord("N")                                     # across the first chunk boundary
    runs[2 * CHUNK - 3:2 * CHUNK] = ord("n")                                    # up to the second one
    for at, b in zip(rng.integers(600_000, 900_000, 40), b"RYKMSWBDHVryu" * 4):
        runs[at] = b
    alternating = variant()
    alternating[0:CHUNK:2] = ord("A")
    alternating[1:CHUNK:2] = ord("N")                                           # 524,288 runs: over any cap
    paths = []
    for k, bases in enumerate((plain, masked, runs, alternating)):
        paths.append(str(tmp / ("doc%d.fa" % k)))
        write_fasta(paths[-1], b"doc%d" % k, bases)
    return tmp, paths


def run_cli(tmp, paths, tag, **env):
    stats = str(tmp / (tag + ".json"))
    r = subprocess.run(["timeout", "-k", "10", "120", EXE] + paths + ["-o", str(tmp / tag)], capture_output=True, text=True,
                       env=dict(os.environ, MUMEMTO_INPUT_CHUNK_MB="1", MUMEMTO_STATS=stats, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    return json.load(open(stats))["input"]


def test_packed_and_raw_input_leave_the_same_files(collection):
    tmp, paths = collection
    stats = {"packed": run_cli(tmp, paths, "packed"), "scalar": run_cli(tmp, paths, "scalar", MUMEMTO_NO_AVX2="1"),
             "raw": run_cli(tmp, paths, "raw", MUMEMTO_NO_CHUNKED_INPUT="1")}
    assert os.path.getsize(tmp / "packed.mums") > 0
    for ext in (".mums", ".lengths"):
        want = (tmp / ("packed" + ext)).read_bytes()
        assert (tmp / ("scalar" + ext)).read_bytes() == want, ext
        assert (tmp / ("raw" + ext)).read_bytes() == want, ext
    for tag in ("packed", "scalar"):
        s = stats[tag]
        print(tag, s)
        assert s["chunks_packed"] > 0
        assert s["chunks_raw"] == 1                        # the alternating stretch is exactly the first chunk of its file
        assert s["chunks_packed"] + s["chunks_raw"] == 4 * ((BASES + CHUNK - 1) // CHUNK)
        assert s["bytes_sent"] < 4 * BASES / 3
        assert s["exception_runs"] >= 5
    assert stats["raw"]["chunks_packed"] == 0 and stats["raw"]["chunks_raw"] == 0
