"""CPU: the plain fold of tests/foldcases.py against the two forms of the reference's fold -- the oracle's restatement
(always) and the reference's own anchor_merge binary (oracle/_ref, when built) -- on built partition sets, and the
conditions the generator has to meet for those sets to be worth folding on the GPU (tests/test_gpu_fold_cases.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import foldcases as F
import pyoracle as O
from mumsfile import format_mums

HERE = os.path.dirname(os.path.abspath(__file__))
REF_MERGE = os.path.join(HERE, "..", "oracle", "_ref", "anchor_merge")
SEEDS = tuple(range(104))
SEEDS32 = (0, 1, 2, 3)
# seeds whose set must hold the named construct (foldcases.CONSTRUCTS; "decider32": of partitions32)
NAMED = {
    "equal": (1, 2, 4, 5, 9, 10, 11, 15),
    "len192021": (1, 2, 4, 5, 7, 9, 10, 11),
    "nested": (4, 5, 7, 9, 10, 11, 14, 15),
    "delta": (4, 5, 9, 10, 11, 14, 19, 20),
    "zero_one_side": (4, 5, 9, 10, 19, 20, 25, 26),
    "first": (0, 6, 12, 24, 30), "last": (0, 1, 2, 4, 5, 6, 7, 9),
    "empty_mid": (3, 13, 23), "empty_last": (8, 18, 28), "decider32": SEEDS32,
}


@functools.lru_cache(maxsize=None)
def case(seed, flavour=16):
    """(parts, anchor length, constructs, fold at min_len 20); flavour 32: partitions32 with its columns saturated, the
    form the reference can read"""
    parts, L, constructs = F.partitions(seed) if flavour == 16 else F.partitions32(seed)
    if flavour == 32:
        parts = F.saturated(parts)
    return parts, L, constructs, F.fold(parts)


CASES = [(s, 16) for s in SEEDS] + [(s, 32) for s in SEEDS32]


def test_fold_equals_the_oracle_restatement():
    for seed, flavour in CASES:
        parts, L, _, (wl, wo, ws, wt) = case(seed, flavour)
        length, off, st, nb = O.anchor_merge(parts)
        assert np.array_equal(length, wl) and np.array_equal(off, wo) and np.array_equal(st, ws), (seed, flavour)
        assert nb.dtype == np.uint16 and np.array_equal(nb, np.minimum(wt, 65535)), (seed, flavour)
        assert np.all(np.diff(wo[:, 0]) > 0), "rows in anchor order, one per anchor position"


def test_oracle_restatement_takes_a_partition_without_rows():
    parts, L, constructs, _ = case(13)
    assert "empty_mid" in constructs and any(len(p[0]) == 0 for p in parts)
    length, off, st, nb = O.anchor_merge(parts)
    assert len(length) == 0 and off.shape == (0, sum(p[1].shape[1] - 1 for p in parts) + 1)
    flat = [(p[0], p[1].reshape(-1), p[2].reshape(-1), p[3]) for p in parts[:2]]      # tables as flat arrays
    assert len(O.anchor_merge(flat + [(np.zeros(0, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.uint8), parts[0][3])])[0]) == 0


@pytest.mark.skipif(not os.path.exists(REF_MERGE), reason="the reference's anchor_merge was not built (oracle/Makefile ref)")
def test_fold_equals_the_reference_binary(tmp_path):
    """The judge: src/merge_candidates.cpp compiled unmodified reads p*.mums / p*.athresh of every set and writes the
    bytes of format_mums(fold rows) and the fold's thresholds.  A partition without rows is a valid input to it: the
    merged file is empty, the thresholds are merged all the same."""
    rows = 0
    for seed, flavour in CASES:
        parts, L, _, (wl, wo, ws, wt) = case(seed, flavour)
        d = tmp_path / ("s%d_%d" % (seed, flavour))
        d.mkdir()
        paths = F.write_set(d, parts)
        r = subprocess.run([REF_MERGE] + paths + ["-o", str(d / "out")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (seed, flavour, r.stderr[-2000:])
        assert (d / "out.mums").read_bytes() == format_mums(wl, wo, ws), (seed, flavour)
        assert np.array_equal(np.fromfile(d / "out.athresh", np.uint16), wt), (seed, flavour)
        rows += len(wl)
    print("reference binary == fold on %d cases, %d merged rows" % (len(CASES), rows))


def test_generator_meets_its_conditions():
    """Not a measurement of anything: the sets are only worth folding if folds of them produce rows and the constructs
    they were built for are in them and come out as designed."""
    counts, seen = [], set()
    for seed in SEEDS:
        parts, L, constructs, (wl, wo, _, _) = case(seed)
        assert L == len(parts[0][3]) and all(len(p[3]) == L for p in parts)
        assert all(len(set(p[1][:, 0].tolist())) == len(p[0]) for p in parts), "anchor starts are distinct"
        assert all(np.all(p[2][:, 0] == 1) for p in parts)
        at = dict(zip(wo[:, 0].tolist(), wl.tolist()))
        for name, want in constructs.items():
            seen.add(name)
            for pos, n in want.items():
                assert at.get(pos, 0) == n, (seed, name, pos, n, at.get(pos, 0))
        if not any(n.startswith("empty") for n in constructs):
            counts.append(len(wl))
        else:
            assert len(wl) == 0 and wo.shape[1] == sum(p[1].shape[1] - 1 for p in parts) + 1
    for name, seeds in NAMED.items():
        for seed in seeds:
            constructs = (F.partitions32(seed) if name == "decider32" else case(seed))[2]
            assert name in constructs, (name, seed)
    assert {len(case(s)[0][0][3]) for s in SEEDS} == set(F.ANCHORS)
    assert max(sum(p[1].shape[1] - 1 for p in case(s)[0]) + 1 for s in SEEDS) == 130
    assert max(int(p[1].max()) for s in SEEDS for p in case(s)[0] if len(p[0])) >= 1 << 40
    print("fold cases: %d sets, %d with rows to make, %d with 10 or more merged rows, %d merged rows; constructs %s"
          % (len(SEEDS), len(counts), sum(c >= 10 for c in counts), sum(counts), sorted(seen)))
    assert 2 * sum(c >= 10 for c in counts) >= len(counts) and sum(counts) >= 500


def test_32_bit_flavour_differs_from_its_saturated_form():
    """partitions32: at least one decider makes a row from the saturated column that the 32-bit column forbids."""
    for seed in SEEDS32:
        parts, L, constructs = F.partitions32(seed)
        assert len(parts) >= 3 and all(p[3].dtype == np.uint32 and int(p[3].max()) > 65535 for p in parts)
        l32, o32, _, t32 = F.fold(parts)
        l16, o16, _, t16 = case(seed, 32)[3]
        only16 = set(o16[:, 0].tolist()) - set(o32[:, 0].tolist())
        assert only16 & {p for p, d in constructs["decider32"].items() if d}, seed
        assert int(t32.max()) > 65535 and np.array_equal(np.minimum(t32, 65535), t16)
        assert int(l32.max()) > 65535
