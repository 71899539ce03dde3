"""CPU: the host model of the MEM density (tests/densmodel.py) against the arrays the reference's tool saved
(tests/golden/density, recorded by tests/golden/make_density.py) and against a plain loop; the binned closed form against the
per-base one summed by bins; mumsio.read_mems against the fixtures; the slice rule the kernels use, on the host; the surface."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import densmodel as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mumemto_amd", "csrc")
ENTRY_POINTS = ["mmt_density_create", "mmt_density_free", "mmt_density_add_rows", "mmt_density_add_engine", "mmt_density_finish",
                "mmt_density_shape", "mmt_density_bins", "mmt_density_bins_device", "mmt_density_stats"]


def widths(size):
    """the bin widths tests/test_gpu_density.py uses"""
    return sorted({w for w in (1, 3, 7, 10, 16, 64, 100, size - 1, size, size + 5) if w >= 1})


@pytest.fixture(scope="module", params=M.FIXTURES)
def fixture(request):
    mems, lens, npy = M.fixture_paths(request.param)
    return request.param, M.read_mems_plain(mems), M.sequence_lengths(lens), np.load(npy)


# ---- the model -------------------------------------------------------------------------------------------------------------
def test_fixtures_are_small_and_hold_their_cases():
    for name in M.FIXTURES:
        for path in M.fixture_paths(name):
            assert os.path.getsize(path) < 100_000, path
        gold = np.load(M.fixture_paths(name)[2])
        assert gold.dtype == np.float64 and gold.shape[0] <= 5 and gold.shape[1] <= 2000
    wraps = np.load(M.fixture_paths("wraps")[2])
    rows = M.read_mems_plain(M.fixture_paths("wraps")[0])
    alone = lambda r: M.per_base(rows[0][r:r + 1], [0, 1], rows[2][rows[1][r]:rows[1][r] + 1], [0], [100, 100])[0]   # noqa: E731
    assert np.nonzero(alone(0))[0].tolist() == list(range(70, 95))         # start -30, l 25
    assert not alone(1).any()                                              # start -1, l 30
    assert np.nonzero(alone(2))[0].tolist() == list(range(95, 100))        # start 95, l 20
    assert np.nonzero(alone(3))[0].tolist() == list(range(0, 30))          # start -120 (below -size), l 150
    assert not alone(4).any()                                              # start -250, l 40
    assert wraps.shape == (2, 100)
    short = np.load(M.fixture_paths("short_seq")[2])
    assert short.shape == (3, 300) and short[1, 120:].any() and short[2, 50:].any()     # covered beyond their own ends
    assert open(M.fixture_paths("multifasta")[1]).read().split()[1] == "*"


def test_model_equals_the_reference_and_the_loop(fixture):
    name, rows, seq_lengths, gold = fixture
    base = M.per_base(*rows, seq_lengths)
    assert base.shape == gold.shape and np.array_equal(base.astype(np.float64), gold), name
    assert np.array_equal(M.loop(*rows, seq_lengths), gold), name


def test_binned_model_equals_the_per_base_one_summed(fixture):
    name, rows, seq_lengths, gold = fixture
    base = M.per_base(*rows, seq_lengths)
    for W in widths(gold.shape[1]):
        got = M.binned(*rows, seq_lengths, W)
        assert got.dtype == np.uint64 and got.shape == (len(seq_lengths), M.nbins_of(gold.shape[1], W))
        assert np.array_equal(got, M.sum_by_bins(base, W)), (name, W)
    assert np.array_equal(M.binned(*rows, seq_lengths, 1), base.astype(np.uint64))


@pytest.mark.parametrize("size,num", [(1, 1), (63, 2), (64, 94), (65, 1), (1000, 2), (100, 3), (95, 3)])
def test_binned_model_on_generator_rows(size, num):
    rows = M.make_rows(seed=1000 * num + size, n_rows=60, num=num, size=size)
    seq_lengths = [size] * num
    base = M.per_base(*rows, seq_lengths)
    if size <= 100:
        assert np.array_equal(M.loop(*rows, seq_lengths), base.astype(np.float64))
    for W in widths(size):
        assert np.array_equal(M.binned(*rows, seq_lengths, W), M.sum_by_bins(base, W)), (size, num, W)
    st = M.stats(*rows, seq_lengths)
    assert st["occurrences"] == len(rows[2]) and (size == 1 or (st["negative"] > 0 and st["cut"] > 0 and st["empty"] > 0))


# ---- the slice rule of the kernels, on the host ------------------------------------------------------------------------------
def test_native_slice_rule(tmp_path):
    from mumemto_amd import build
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "density_check")
    hip_include = os.path.join(os.path.dirname(os.path.dirname(build.HIPCC)), "include")
    # (the sanitizers' runtimes inside the program: it runs as it is, whatever the environment preloads)
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-isystem", hip_include,
                    os.path.join(HERE, "density_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(5)
    cases = [(-30, 25, 100), (-1, 30, 100), (95, 20, 100), (100, 0, 100), (100, 5, 100), (101, 0, 100), (80, 20, 100), (80, 21, 100),
             (-100, 100, 100), (-101, 1, 100), (-250, 40, 100), (-120, 150, 100), (0, 0, 1), (0, 1, 1), (-1, 1, 1), (-1, 2, 1),
             (2 ** 63 - 1, 2 ** 32 - 1, 1 << 40), (-2 ** 63, 2 ** 32 - 1, 1 << 40), (-2 ** 63 + (1 << 40), 7, 1 << 40),
             ((1 << 40) - 1, 2 ** 32 - 1, 1 << 40), (-1, 2 ** 32 - 1, 1 << 40)]
    for size in (1, 2, 64, 1000):
        cases += [(int(s), int(l), size) for s, l in zip(rng.integers(-3 * size - 2, 2 * size + 3, 300), rng.integers(0, 2 * size + 3, 300))]
    r = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (start, l, size), (a, b, cut) in zip(cases, got):
        # Python's own arithmetic (no overflow) and, at small sizes, numpy's slice itself
        stop = start + l
        wa = max(start + size, 0) if start < 0 else min(start, size)
        wb = max(stop + size, 0) if stop < 0 else min(stop, size)
        assert (max(b - a, 0), cut) == (max(wb - wa, 0), int(stop > size)), (start, l, size, a, b, cut)
        assert wa >= wb or (a, b) == (wa, wb), (start, l, size, a, b)
        if size <= 1000:
            assert np.arange(size)[start:stop].tolist() == list(range(a, b)), (start, l, size, a, b)


# ---- read_mems ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_occ", [1, 2, 5, 64, 1 << 24])
def test_read_mems_batches(fixture, max_occ):
    from mumemto_amd import mumsio
    name, rows, _, _ = fixture
    batches = list(mumsio.read_mems(M.fixture_paths(name)[0], max_occ))
    for lengths, occ_start, starts, docs in batches:
        assert (lengths.dtype, occ_start.dtype, starts.dtype, docs.dtype) == (np.uint32, np.uint64, np.int64, np.uint64)
        assert occ_start[0] == 0 and occ_start[-1] == len(starts) == len(docs) and len(occ_start) == len(lengths) + 1
        assert (np.diff(occ_start.astype(np.int64)) >= 1).all() and (len(starts) <= max_occ or len(lengths) == 1)
    assert np.array_equal(np.concatenate([b[0] for b in batches]), rows[0])
    assert np.array_equal(np.concatenate([b[2] for b in batches]), rows[2])
    assert np.array_equal(np.concatenate([b[3] for b in batches]), rows[3])
    counts = np.concatenate([np.diff(b[1].astype(np.int64)) for b in batches])
    assert np.array_equal(counts, np.diff(rows[1].astype(np.int64)))
    if max_occ >= len(rows[2]):
        assert len(batches) == 1


def test_read_mems_refuses_malformed_lines(tmp_path):
    from mumemto_amd import mumsio
    good = "25\t-30,10\t0,1\t+,-\n\n30\t5,6,7\t0,1,1\t+,-,+\n"
    path = str(tmp_path / "x.mems")
    open(path, "w").write(good)
    (a, b, c, d), = list(mumsio.read_mems(path))                       # (a blank line is skipped, and counted)
    assert a.tolist() == [25, 30] and b.tolist() == [0, 2, 5] and c.tolist() == [-30, 10, 5, 6, 7] and d.tolist() == [0, 1, 0, 1, 1]
    for bad, message in (("20\t1,2,3\t0,1\t+,+,+\n", r"line 4: 3 starts but 2 documents"),
                         ("20\t1,2\t0,1,2\t+,+\n", r"line 4: 2 starts but 3 documents"),
                         ("20\t1,2\n", r"line 4: fewer than three fields"),
                         ("20\t1,x\t0,1\t+,+\n", r"line 4: field 2 .* no integer"),
                         ("20\t1,,2\t0,1,1\t+,+\n", r"line 4: field 2 .* no integer"),
                         ("-20\t1,2\t0,1\t+,+\n", r"line 4: a length outside"),
                         ("20\t1,2\t0,-1\t+,+\n", r"line 4: a length outside \[0, 2\^32\) or a negative document")):
        open(path, "w").write(good + bad)
        with pytest.raises(ValueError, match=message):
            list(mumsio.read_mems(path, 2))
    assert "silently drops the tail" in mumsio.read_mems.__doc__
    open(path, "w").write("")
    assert list(mumsio.read_mems(path)) == []


# ---- the surface -------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_and_documented():
    from mumemto_amd import binding
    header = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    api = open(os.path.join(CSRC, "api.cpp")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"MMT_API [\w\s\*]+\b%s\(" % name, header), name
        assert re.search(r"\b%s\(" % name, api), name
        assert name in binding.GPU_ABI_SYMBOLS, name
    assert "mumemto/mem_density.py" in header
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "mem_density" in open(os.path.join(ROOT, doc)).read(), doc
    import mumemto_amd
    assert callable(mumemto_amd.mem_density) and "mem_density" in dir(mumemto_amd) and "Density" in dir(mumemto_amd)
    for method in ("add_rows", "add_engine", "finish", "bins", "bins_device", "stats", "close", "__enter__", "__exit__"):
        assert callable(getattr(mumemto_amd.Density, method)), method
    assert callable(mumemto_amd.Engine.mem_density)


def test_build_lists_the_sources():
    from mumemto_amd import build
    assert "density.cpp" in build.LIB_SOURCES and "density_kernels.hip" in build.LIB_SOURCES
    for f in ("density.cpp", "density.hpp", "density_kernels.hip", "density_kernels.hpp"):
        assert os.path.exists(os.path.join(CSRC, f)), f
    kernels = open(os.path.join(CSRC, "density_kernels.hip")).read()
    assert "grid_capped(" in kernels and "launch_grid.hpp" in kernels
    assert re.search(r"#define DENSITY_PREAGG 1", open(os.path.join(CSRC, "density_kernels.hpp")).read())


def test_tool_arguments():
    from mumemto_amd.mem_density import parse_arguments
    r = subprocess.run([sys.executable, "-m", "mumemto_amd.mem_density", "--help"], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 0 and b"--bin" in r.stdout and b"--device" in r.stdout      # (argparse leaves before the library loads)
    a = parse_arguments(["-m", "x/run.mems", "-l", "x/run.lengths"])
    assert (a.mems, a.lengths, a.verbose, a.bin, a.output) == ("x/run.mems", "x/run.lengths", False, 1, None)
    a = parse_arguments(["--mems", "r.mems", "--lengths", "r.lengths", "-v", "--bin", "1000", "-o", "out.npy", "--device", "3"])
    assert (a.verbose, a.bin, a.output, a.device) == (True, 1000, "out.npy", 3)
