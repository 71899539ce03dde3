"""The string fold on the device (mumemto_amd/csrc/string_fold.cpp), host side: its surface, and the inputs and checks of
tests/test_gpu_string_fold.py held to the closed form alone (mumemto_amd/merge_mums.py string_merge, which
tests/test_string_merge_host.py holds to the reference's own files).  No GPU."""
import os
import re

import numpy as np
import pytest

import stringfold_cases as SC
from mumemto_amd import binding, merge_mums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mmt_string_fold", "mmt_merged_string_thresh", "mmt_merged_string_thresh_device", "mmt_merged_string_thresh_len",
                "mmt_merged_string_fold_stats")


@pytest.fixture(scope="module")
def modelled():
    """name -> (inputs, the closed form's five results, the trace), computed once and left as they are"""
    out = {}
    for name in SC.NAMED:
        parts, mom, records = SC.named_case(name)
        out[name] = ((parts, mom, records), merge_mums.string_merge(parts, mom, records), SC.trace(parts, mom, records))
    return out


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "mumemto_gpu.h")).read()
    sig = lambda s: re.search(r"\s*".join(re.escape(tok) for tok in s.split(" ")), text)      # noqa: E731
    assert sig("MMT_API int mmt_string_fold(mmt_engine* e, const mmt_string_part* parts, size_t S, const mmt_string_part* mom, "
               "const mmt_string_records* mom_records, mmt_merged** out)")
    assert sig("MMT_API int mmt_merged_string_thresh(const mmt_merged* m, uint16_t* thresh, uint16_t* thresh_rev)")
    assert sig("MMT_API int mmt_merged_string_thresh_device(const mmt_merged* m, const uint16_t** thresh, const uint16_t** thresh_rev)")
    assert sig("MMT_API uint64_t mmt_merged_string_thresh_len(const mmt_merged* m)")
    assert sig("MMT_API int mmt_merged_string_fold_stats(const mmt_merged* m, double out[8])")
    assert "typedef struct mmt_string_part" in text and "typedef struct mmt_string_records" in text
    assert "input # of MUM files does not match merged MUM input file" in text
    api = open(os.path.join(ROOT, "mumemto_amd", "csrc", "api.cpp")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, api), name
        assert name in binding.GPU_ABI_SYMBOLS, name


def test_sources_and_documents():
    from mumemto_amd import build
    assert "string_fold.cpp" in build.LIB_SOURCES and "string_fold_kernels.hip" in build.LIB_SOURCES
    for f in ("string_fold.cpp", "string_fold.hpp", "string_fold_kernels.hip", "string_fold_kernels.hpp"):
        assert os.path.exists(os.path.join(ROOT, "mumemto_amd", "csrc", f)), f
    consts = open(os.path.join(ROOT, "mumemto_amd", "csrc", "string_fold_kernels.hpp")).read()
    block = int(re.search(r"THRESH_BLOCK\s*=\s*(\d+)", consts).group(1))
    per_item = int(re.search(r"THRESH_PER_ITEM\s*=\s*(\d+)", consts).group(1))
    assert block * per_item == SC.TILE                                  # the tile the cases place their row lengths around
    assert int(re.search(r"MIN_SEGMENT\s*=\s*(\d+)", consts).group(1)) == SC.MIN_SEGMENT == merge_mums.MIN_SEGMENT
    assert int(re.search(r"THRESH_MAX_ROWS\s*=\s*(\d+)", consts).group(1)) == SC.MAX_ROWS     # what the many-rows cases are sized by
    assert eval(re.search(r"THRESH_LDS_BYTES\s*=\s*([\d *]+);", consts).group(1)) == SC.LDS_BYTES
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "string_fold" in open(os.path.join(ROOT, doc)).read(), doc


def test_python_surface():
    import mumemto_amd
    assert callable(mumemto_amd.string_merge_device) and "string_merge_device" in dir(mumemto_amd)
    for method in ("string_fold", "string_thresh", "string_thresh_device", "string_fold_stats"):
        assert callable(getattr(mumemto_amd.Merged, method)), method
    assert [f[0] for f in binding.StringPart._fields_] == ["n_rows", "n_docs", "length", "starts", "strands", "thresh", "thresh_rev",
                                                            "thresh_len"]
    assert [f[0] for f in binding.StringRecords._fields_] == ["n_collections", "begin", "length"]
    args = merge_mums.parse_arguments(["a.mums", "b.mums"])
    assert args.device is False                                        # the default stays the closed form on the host
    assert merge_mums.parse_arguments(["--device", "a.mums", "b.mums"]).device is True


# ---- the inputs: the model alone reaches what every case is named for ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.NAMED))
def test_the_model_reaches_the_boundary_of_the_case(modelled, name):
    (parts, mom, records), want, tr = modelled[name]
    assert SC.NAMED[name][1](tr, parts, want), name
    assert SC.counts(tr)["rows"] == len(want[0])                       # the trace and the closed form speak of the same pieces
    if name != "empty":
        assert len(want[0]) >= 1
    # what the fold requires of its inputs
    for (lengths, starts, strands, th, th_rev), rec in zip(parts, records):
        assert (np.diff(starts[:, 0]) >= 0).all() and (starts != -1).all()
        assert len(th) == len(th_rev) == int((lengths.astype(np.int64) + 1).sum())
        assert len(rec) == len(lengths) and rec[-1] < lengths[-1] + 1 and (rec[:-1] == lengths[:-1].astype(np.int64) + 1).all()
    assert (mom[1] != -1).all()
    assert len(want[3]) == len(want[4]) == int(want[0].astype(np.int64).sum()) + len(want[0])


def test_the_lengths_of_the_tile_case_straddle_the_tiles(modelled):
    _, want, _ = modelled["tile_edges"]
    begins = np.cumsum(want[0].astype(np.int64) + 1) - want[0] - 1      # first output position of every row
    ends = begins + want[0]                                             # its terminating 0
    assert len(want[3]) > 3 * SC.TILE
    assert any(b // SC.TILE + 2 <= e // SC.TILE for b, e in zip(begins, ends))          # a row over a whole tile and into the next
    assert any(b % SC.TILE == 0 for b in begins[1:]) or any(b // SC.TILE != e // SC.TILE for b, e in zip(begins, ends))


def test_a_quarter_of_the_sweeps_pieces_survive():
    pieces = rows = multi = reversed_ = 0
    for seed in SC.SWEEP_SEEDS:
        parts, mom, records = SC.random_case(seed)
        tr = SC.trace(parts, mom, records)
        want = merge_mums.string_merge(parts, mom, records)
        c = SC.counts(tr)
        assert c["rows"] == len(want[0]), seed
        pieces += c["pieces"]
        rows += c["rows"]
        multi += sum(p["of"] > 1 for p in tr)
        reversed_ += sum(p["kept"] and not all(q["forward"] for q in p["parts"]) for p in tr)
        assert len(want[3]) < 400000
    assert 4 * rows >= pieces > 2000
    assert multi > 200 and reversed_ > 200


# ---- the checks reject what is wrong --------------------------------------------------------------------------------------------
def test_the_checks_reject_a_wrong_output(modelled):
    _, want, tr = modelled["four_signs"]
    SC.check_fold(tuple(a.copy() for a in want), want)
    SC.check_counts(SC.counts(tr), tr)

    def wrong(change):
        got = [a.copy() for a in want]
        change(got)
        with pytest.raises(AssertionError):
            SC.check_fold(tuple(got), want)

    def off_by_one(got):
        got[1][2, 3] += 1

    def swapped_files(got):
        at = int(np.nonzero(got[3] != got[4])[0][0])
        got[3][at], got[4][at] = got[4][at], got[3][at]

    def rows_exchanged(got):
        for a in got[:3]:
            a[[0, 1]] = a[[1, 0]]

    def flipped_strand(got):
        got[2][1, 0] = not got[2][1, 0]

    def narrower(got):
        got[3] = got[3].astype(np.uint32)

    for change in (off_by_one, swapped_files, rows_exchanged, flipped_strand, narrower):
        wrong(change)
    with pytest.raises(AssertionError):
        SC.check_fold(tuple(a[:-1] for a in want), want)
    bad = dict(SC.counts(tr))
    bad["dropped_short"] += 1
    with pytest.raises(AssertionError):
        SC.check_counts(bad, tr)
