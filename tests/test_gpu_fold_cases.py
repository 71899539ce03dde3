"""GPU: the anchor fold (merge.cpp, merge_kernels.hip, k_fold_step) on the built partition sets of tests/foldcases.py,
against foldcases.fold -- the plain fold that tests/test_fold_host.py holds to the reference's own anchor_merge binary on
the same sets.  Every comparison is exact: rows, strands, thresholds, and the bytes of the merged .mums."""
import functools
import os
import subprocess

import numpy as np
import pytest

import foldcases as F
import pyoracle as O
from mumsfile import format_mums

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BIN_MERGE = os.path.join(HERE, "..", "mumemto_amd", "bin", "anchor_merge")
REF_MERGE = os.path.join(HERE, "..", "oracle", "_ref", "anchor_merge")
SEEDS = tuple(range(36)) + (39,)        # every anchor length six times, five sets with a partition without rows, 130 columns
SEEDS32 = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def case(seed):
    return F.partitions(seed)


@functools.lru_cache(maxsize=None)
def want(seed, min_len=20):
    return F.fold(case(seed)[0], min_len)


def same(got, ref, tag, text=True):
    wl, wo, ws, wt = ref
    assert got["n_rows"] == len(wl) and got["n_docs"] == wo.shape[1], tag
    assert np.array_equal(got["lengths"], wl), tag
    assert got["offsets"].shape == wo.shape and np.array_equal(got["offsets"], wo), tag
    assert np.array_equal(got["strands"], ws), tag
    assert got["thresh"].dtype == np.uint16 and np.array_equal(got["thresh"], np.minimum(wt, 65535)), tag
    if text:
        assert got["text"] == format_mums(wl, wo, ws), tag


def wide(parts):
    return [(p[0], p[1], p[2], p[3].astype(np.uint32)) for p in parts]


def on_device(parts):
    """rows and thresholds in device memory, as the multi-GPU exchange hands them to the fold"""
    import torch
    from mumemto_amd import dist as mdist
    from mumemto_amd.binding import DevicePartition
    dev = torch.device("cuda", 0)
    out = []
    for p in parts:
        t = (torch.from_numpy(p[0].view(np.int32)).to(dev), torch.from_numpy(p[1]).to(dev), torch.from_numpy(p[2]).to(dev),
             torch.from_numpy(p[3].view(np.int32 if p[3].dtype == np.uint32 else np.int16)).to(dev))
        if p[3].dtype == np.uint32:
            out.append(DevicePartition(t[1].shape[0], t[1].shape[1], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                       t[3].data_ptr(), t[3].numel(), keepalive=t, thresh_bits=32))
        else:
            out += mdist.device_partitions([t])
    return out


@pytest.mark.parametrize("where", ["host", "device"])
def test_whole_fold(where):
    """Engine.anchor_merge == fold for min_len 1, 20 and 50, from 16-bit and from 32-bit threshold columns, partitions
    in host memory and in device memory."""
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    try:
        rows = 0
        for seed in SEEDS:
            parts = case(seed)[0]
            for flavour in (parts, wide(parts)):
                use = on_device(flavour) if where == "device" else flavour
                for min_len in (1, 20, 50):
                    same(eng.anchor_merge(use, min_len=min_len), want(seed, min_len), (seed, min_len, flavour[0][3].dtype))
            rows += len(want(seed)[0])
        assert rows >= 500
    finally:
        eng.close()


def test_32_bit_thresholds_decide_where_16_bits_saturate():
    """foldcases.partitions32: merged lengths and thresholds of 65,535 .. 70,001 on the deciding positions.  The fold of
    the 32-bit columns is fold's; of the same columns saturated to 16 bits it is fold's of those, which holds rows the
    first must not."""
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    try:
        for seed in SEEDS32:
            parts, L, constructs = F.partitions32(seed)
            w32, w16 = F.fold(parts), F.fold(F.saturated(parts))
            deciders = {p for p, d in constructs["decider32"].items() if d}
            for where in ("host", "device"):
                g32 = eng.anchor_merge(on_device(parts) if where == "device" else parts)
                g16 = eng.anchor_merge(on_device(F.saturated(parts)) if where == "device" else F.saturated(parts))
                same(g32, w32, (seed, where, 32))
                same(g16, w16, (seed, where, 16))
                assert (set(g16["offsets"][:, 0].tolist()) - set(g32["offsets"][:, 0].tolist())) & deciders, (seed, where)
            same(eng.anchor_merge(parts, slices=3), w32, (seed, "slices"))
            for min_len in (1, 50):
                same(eng.anchor_merge(parts, min_len=min_len), F.fold(parts, min_len), (seed, min_len))
    finally:
        eng.close()


def _range_fold(seeds):
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    try:
        for seed in seeds:
            parts, L, _ = case(seed)
            assert max(int(p[0].max()) for p in parts if len(p[0])) > L // 64, "a row longer than a slice"
            whole = eng.anchor_merge(parts)
            same(whole, want(seed), (seed, "whole"))
            for where in ("host", "device") if seed % 4 == 0 and L <= 257 else ("host",):
                use = on_device(parts) if where == "device" else parts
                for s in (1, 2, 3, 7, 64, L + 5):
                    got = eng.anchor_merge(use, slices=s)
                    for key in ("lengths", "offsets", "strands", "thresh"):
                        assert np.array_equal(got[key], whole[key]), (seed, where, s, key)
                    assert got["text"] == whole["text"], (seed, where, s)
    finally:
        eng.close()


def test_range_fold_small_anchors():
    """anchor_merge(parts, slices=s) == the whole fold for s = 1, 2, 3, 7, 64 and anchor length + 5 (most slices empty,
    the first ones of no anchor position at all), on the anchors of 40, 256 and 257 (every fourth set from device memory
    too): rows of 300 span many slices, sets 13 and 8 / 18 hold a partition without rows."""
    seeds = tuple(s for s in SEEDS if case(s)[1] <= 257 and len(case(s)[0]) <= 6)
    assert {13, 8, 18} <= set(seeds)
    _range_fold(seeds)


@pytest.mark.parametrize("seed", [3, 4])
def test_range_fold_anchors_of_4096_and_4097(seed):
    """The same on an anchor of 4,096 (set 3: a partition without rows in the middle) and one of 4,097 (set 4)."""
    _range_fold((seed,))


def test_table_writer_up_to_130_columns():
    """k_table_write formats 64 cells a pass: 2, 64, 65 and 130 output columns (1 + 0 + 1: a partition of the anchor
    alone; 1 + 3 x 21, 1 + 4 x 16, 1 + 43 x 3), offsets of 1 to 13 digits."""
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    try:
        digits = set()
        for cols, further in ((2, [0, 1]), (64, [21] * 3), (65, [16] * 4), (130, [3] * 43)):
            parts, L, _ = F.partitions(100 + cols, further=further, anchor_len=257)
            ref = F.fold(parts)
            assert ref[1].shape[1] == cols and len(ref[0]) >= 5
            digits |= {len(str(int(x))) for x in ref[1].reshape(-1)}
            same(eng.anchor_merge(parts), ref, cols)
            same(eng.anchor_merge(on_device(parts), slices=3), ref, cols)
        assert digits >= set(range(1, 14))
    finally:
        eng.close()


def test_resort_orders_rows_by_the_anchor_suffix_rank():
    """anchor_merge(sort_like_direct=True): the fold's rows ordered by the rank of the text suffix at their anchor offset.
    The engine holds the ranks of its last run (two small documents, merge metadata on); the expected ranks come from
    the oracle's suffix array of the same text, whose first positions are the anchor's forward strand."""
    import mumemto_amd
    from mumemto_amd import synth
    docs = synth.pangenome(2, 1531, 0.02, seed=5)
    L0 = len(docs[0][0])
    text, _ = O.build_text(docs, True)
    sa, _, _ = O.build_stream(text)
    rank = np.zeros(len(text) + 1, np.int64)
    rank[sa] = np.arange(len(sa))
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_docs(docs)
        eng.run(merge_metadata=True)
        for seed in (4, 5, 9, 11, 3):
            parts, L, _ = F.partitions(seed, anchor_len=L0)
            wl, wo, ws, wt = F.fold(parts)
            order = np.argsort(rank[wo[:, 0]], kind="stable")
            assert seed == 3 or (len(wl) >= 10 and not np.array_equal(order, np.arange(len(wl))))
            for use in (parts, on_device(parts)):
                same(eng.anchor_merge(use, sort_like_direct=True), (wl[order], wo[order], ws[order], wt), seed)
            same(eng.anchor_merge(parts, sort_like_direct=True, slices=7), (wl[order], wo[order], ws[order], wt), seed)
    finally:
        eng.close()


def test_command_line_tool(tmp_path):
    """mumemto_amd/bin/anchor_merge p*.mums -o out: out.mums / out.athresh are the fold's, and byte for byte what the
    reference's tool writes from the same files when it is there.  Rows are in shuffled order in every file; sets 3, 13
    and 8 hold a partition without rows (an empty .mums file: an empty merged file, thresholds merged all the same);
    set 39 has 43 partitions."""
    for seed in (1, 4, 3, 13, 8, 39):
        parts = case(seed)[0]
        wl, wo, ws, wt = want(seed)
        d = tmp_path / ("s%d" % seed)
        d.mkdir()
        paths = F.write_set(d, parts)
        assert any(np.any(np.diff(p[1][:, 0]) < 0) for p in parts if len(p[0]))
        r = subprocess.run([BIN_MERGE] + paths + ["-o", str(d / "out")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (seed, r.stderr[-2000:])
        assert (d / "out.mums").read_bytes() == format_mums(wl, wo, ws), seed
        assert np.array_equal(np.fromfile(d / "out.athresh", np.uint16), np.minimum(wt, 65535)), seed
        if os.path.exists(REF_MERGE):
            r = subprocess.run([REF_MERGE] + paths + ["-o", str(d / "ref")], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (seed, r.stderr[-2000:])
            assert (d / "out.mums").read_bytes() == (d / "ref.mums").read_bytes(), seed
            assert (d / "out.athresh").read_bytes() == (d / "ref.athresh").read_bytes(), seed
