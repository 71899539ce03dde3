"""The string fold on the device (mumemto_amd/csrc/string_fold.cpp: rows and thresholds of the string-based merge's last step)
against the closed form, mumemto_amd/merge_mums.py string_merge, and against the files the reference's own tools wrote
(tests/golden/string_merge).  Every comparison is exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import stringfold_cases as SC
from mumemto_amd import binding, build, merge_mums, mumsio, synth

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(build.LIB), "..", "bin")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "string_merge")
GOLDEN = sorted(os.listdir(GOLD))
MISMATCH = "input # of MUM files does not match merged MUM input file"


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def engine():
    eng = binding.Engine(0)
    yield eng
    eng.close()


def fold(engine, parts, mom, records):
    """-> (the five results, the stats) of one fold on the device"""
    with binding.Merged.string_fold(engine, parts, mom, records) as m:
        length, starts, strands = m.rows()
        return (length, starts, strands.astype(bool)) + m.string_thresh(), m.string_fold_stats()


@pytest.fixture
def golden_dir(tmp_path, request):
    dst = tmp_path / request.param
    shutil.copytree(os.path.join(GOLD, request.param), dst)
    cwd = os.getcwd()
    os.chdir(dst)
    yield ["p%d.mums" % g for g in range(len([f for f in os.listdir(dst) if f.startswith("p") and f.endswith(".mums")]))]
    os.chdir(cwd)


# ---- the reference's own files ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("golden_dir", GOLDEN, indirect=True)
def test_golden_cases_through_the_free_function(golden_dir):
    parts = []
    for f in golden_dir:
        p = f[:-5]
        parts.append(mumsio.read_mums(f) + (np.fromfile(p + ".thresh", np.uint16), np.fromfile(p + ".thresh_rev", np.uint16)))
    mom, records = mumsio.read_mums("mom.mums"), merge_mums.record_lengths("mom.lengths")
    got = binding.string_merge_device(parts, mom, records)
    SC.check_fold(got, merge_mums.string_merge(parts, mom, records))
    mumsio.write_mums("ours.mums", *got[:3])
    mumsio.write_bumbl("ours_bin.bumbl", *got[:3])
    assert read("ours.mums") == read("merged.mums") and read("ours_bin.bumbl") == read("merged_bin.bumbl")
    assert got[3].tobytes() == read("merged.thresh") and got[4].tobytes() == read("merged.thresh_rev")


@pytest.mark.parametrize("golden_dir", GOLDEN, indirect=True)
def test_golden_cases_through_the_tool(golden_dir):
    n = merge_mums.main(merge_mums.parse_arguments(["--device", "-m", "mom.mums", "-o", "ours"] + golden_dir))
    for ext in (".mums", ".thresh", ".thresh_rev", ".lengths"):
        assert read("ours" + ext) == read("merged" + ext), ext
    assert n == len(read("merged.mums").splitlines())
    merge_mums.main(merge_mums.parse_arguments(["-m", "mom", "-o", "ours_bin.bumbl", "--device"] + golden_dir))
    assert read("ours_bin.bumbl") == read("merged_bin.bumbl")
    for ext in (".thresh", ".thresh_rev"):
        assert read("ours_bin" + ext) == read("merged" + ext), ext


# ---- the closed form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.NAMED))
def test_named_cases_equal_the_model(engine, name):
    parts, mom, records = SC.named_case(name)
    got, stats = fold(engine, parts, mom, records)
    SC.check_fold(got, merge_mums.string_merge(parts, mom, records), name)
    SC.check_counts(stats, SC.trace(parts, mom, records), name)
    assert all(stats[k] >= 0.0 for k in ("split_ms", "locate_ms", "assemble_ms", "thresholds_ms"))


@pytest.mark.parametrize("seed", SC.SWEEP_SEEDS)
def test_the_sweep_equals_the_model(engine, seed):
    parts, mom, records = SC.random_case(seed)
    got, stats = fold(engine, parts, mom, records)
    SC.check_fold(got, merge_mums.string_merge(parts, mom, records), "seed %d" % seed)
    SC.check_counts(stats, SC.trace(parts, mom, records), "seed %d" % seed)


def test_the_result_is_a_merged_table_like_any_other(engine):
    parts, mom, records = SC.named_case("four_signs")
    want = merge_mums.string_merge(parts, mom, records)
    with binding.Merged.string_fold(engine, parts, mom, records) as m:
        assert (m.n_rows, m.n_docs) == want[1].shape
        lines = m.text().decode().splitlines()
        assert [int(ln.split("\t")[0]) for ln in lines] == want[0].tolist()
        assert [[int(x) for x in ln.split("\t")[1].split(",")] for ln in lines] == want[1].tolist()
        a, b, n = m.string_thresh_device()
        assert a and b and a != b and n == len(want[3])
        m.collinear(1000, None)                                       # replaces the table: the thresholds of the old order go
        with pytest.raises(binding.MumemtoError, match="no merged thresholds attached"):
            m.string_thresh()
        assert int(m.L.mmt_merged_string_thresh_len(m.h)) == 0
    with binding.Merged.from_rows(engine, *want[:3]) as plain:
        with pytest.raises(binding.MumemtoError, match="no merged thresholds attached"):
            plain.string_thresh()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def refused(engine, message, parts, mom, records):
    with pytest.raises(binding.MumemtoError, match=message) as err:
        binding.Merged.string_fold(engine, parts, mom, records)
    assert "rc=3" in str(err.value)
    good = SC.named_case("cut_0_1_3")                                 # the engine is as usable as before
    SC.check_fold(fold(engine, *good)[0], merge_mums.string_merge(*good), "after a refusal")


def changed(case, part=None, **fields):
    """the case with fields of one partition (or of mom: part None) replaced; fields by position in the tuple"""
    parts, mom, records = case
    parts = [tuple(a.copy() for a in p) for p in parts]
    mom = tuple(a.copy() for a in mom)
    target = list(mom if part is None else parts[part])
    for k, v in fields.items():
        target[int(k[1:])] = v(target[int(k[1:])])
    if part is None:
        return parts, tuple(target), records
    parts[part] = tuple(target)
    return parts, mom, records


def test_counts_that_do_not_match_are_refused_in_the_models_words(engine):
    parts, mom, records = SC.named_case("cols_2_2_2")
    with pytest.raises(ValueError, match=MISMATCH):
        merge_mums.string_merge(parts[:2], mom, records)
    refused(engine, MISMATCH, parts[:2], mom, records)                # S = 2 against three columns and three collections
    refused(engine, MISMATCH, parts, mom, records[:2])                # two collections
    refused(engine, MISMATCH, parts, (mom[0], mom[1][:, :2], mom[2][:, :2]), records)


def test_absent_starts_are_refused(engine):
    case = SC.named_case("cols_1_3")

    def absent(at):
        def change(a):
            a[at] = -1
            return a
        return change
    refused(engine, r"partition 1 has an absent start \(-1\)", *changed(case, 1, f1=absent((2, 2))))
    refused(engine, r"partition 0 has an absent start \(-1\)", *changed(case, 0, f1=absent((0, 0))))
    refused(engine, r"the MUMs of MUMs has an absent start \(-1\)", *changed(case, None, f1=absent((3, 1))))


def test_partitions_out_of_order_and_tables_of_another_length_are_refused(engine):
    case = SC.named_case("cut_0_1_3")

    def exchanged(a):
        a[[2, 3]] = a[[3, 2]]
        return a
    refused(engine, "the rows of partition 1 are not in the order of their first column", *changed(case, 1, f1=exchanged))
    T = len(case[0][0][3])
    refused(engine, "the threshold tables of partition 0 hold %d entries, its rows %d positions" % (T - 1, T),
            *changed(case, 0, f3=lambda a: a[:-1], f4=lambda a: a[:-1]))
    refused(engine, "the threshold tables of partition 1 hold %d entries, its rows %d positions" % (T + 2, T),
            *changed(case, 1, f3=lambda a: np.concatenate((a, a[:2])), f4=lambda a: np.concatenate((a, a[:2]))))
    with pytest.raises(binding.MumemtoError, match="thresh and thresh_rev of a partition differ in length"):
        binding.Merged.string_fold(engine, *changed(case, 0, f3=lambda a: a[:-1]))


def test_records_that_cannot_be_are_refused(engine):
    parts, mom, records = SC.named_case("cut_0_1_3")
    more = [records[0], np.concatenate((records[1], [5]))]
    refused(engine, "collection 1 has 9 records, partition 1 only 8 rows", parts, mom, more)
    negative = [records[0].copy(), records[1]]
    negative[0][3] = -2
    refused(engine, "record 3 of collection 0 has a negative length", parts, mom, negative)


def test_too_many_rows_and_too_many_pieces_are_refused(engine):
    # 2^32 rows: the count alone is judged, before a table is touched
    parts, mom, records = SC.named_case("cut_0_1_3")
    L = engine.L
    keep = []

    def struct(rows, th=None, th_rev=None, n_rows=None):
        arrays = [np.ascontiguousarray(rows[0], np.uint32), np.ascontiguousarray(rows[1], np.int64),
                  np.ascontiguousarray(rows[2], np.uint8)] + [np.ascontiguousarray(t if t is not None else [], np.uint16) for t in (th, th_rev)]
        keep.extend(arrays)
        return binding.StringPart(len(arrays[0]) if n_rows is None else n_rows, arrays[1].shape[1], *[a.ctypes.data for a in arrays],
                                  len(arrays[3]))
    begin = np.array([0, len(records[0]), len(records[0]) + len(records[1])], np.uint64)
    flat = np.concatenate(records).astype(np.int64)
    rec = binding.StringRecords(2, begin.ctypes.data, flat.ctypes.data)
    for which in (0, 1, 2):
        arr = (binding.StringPart * 2)(*[struct(p[:3], p[3], p[4], (1 << 32) if which == i else None) for i, p in enumerate(parts)])
        mom_s = struct(mom, n_rows=(1 << 32) - 1 if which == 2 else None)
        out = C.c_void_p()
        assert L.mmt_string_fold(engine.h, arr, 2, C.byref(mom_s), C.byref(rec), C.byref(out)) == 3 and not out.value
        what = b"the MUMs of MUMs" if which == 2 else b"partition %d" % which
        assert what in L.mmt_last_error() and b"rows: 2^32 - 1 or more are not supported" in L.mmt_last_error()
    # 2^32 pieces: 70,000 rows of mom that each span the 70,000 one-base records of collection 0 (n + 1 pieces each)
    n = 70000
    rng = np.random.default_rng(5)
    made = [SC.make_part(rng, np.ones(n, np.uint32), 1, gap=0) for _ in range(2)]
    big_mom = (np.full(n, 2 * n, np.uint32), np.zeros((n, 2), np.int64), np.ones((n, 2), bool))
    refused(engine, r"cut into 2\^32 - 256 pieces or more \(%d\)" % (n * (n + 1)), [m[0] for m in made], big_mom, [m[1] for m in made])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_the_tool_with_the_device_equals_the_tool_without(tmp_path):
    docs = synth.pangenome(9, 200000, 0.004, seed=77, indel_rate=0.001, inversion=(4, 50000, 90000))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for i, d in enumerate(docs):
            synth.write_fasta("h%d.fa" % i, d)
        groups = [[0, 1, 2], [4, 3, 5], [6, 7, 8]]                # as tests/test_gpu_string_merge.py: partition 1 starts inverted
        for g, members in enumerate(groups):
            r = subprocess.run([os.path.join(BIN, "mumemto_exec")] + ["h%d.fa" % i for i in members] + ["-M", "-o", "part%d" % g],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            merge_mums.sort_partition("part%d" % g)
        files = ["part%d.mums" % g for g in range(3)]
        n_dev = merge_mums.main(merge_mums.parse_arguments(files + ["-o", "dev.mums", "--device"]))
        n_host = merge_mums.main(merge_mums.parse_arguments(files + ["-o", "host.mums"]))
        assert n_dev == n_host > 1000
        for ext in (".mums", ".thresh", ".thresh_rev", ".lengths"):
            assert read("dev" + ext) == read("host" + ext), ext
        assert not [f for f in os.listdir(".") if "_temp_merged" in f or f.endswith("_mums.fa")]
    finally:
        os.chdir(cwd)
