"""The launch wrappers of csrc/guided_kernels.hpp (mmt::gk, the bucket-wise producer), one at a time, against the plain
integer model of tests/guidedmodel.py: exact comparison, sentinels behind and between everything a wrapper may write,
cases (tests/guided_cases.py) at the boundaries the kernels' code names.  tests/test_guided_model_host.py checks the model,
the cases and the census of wrappers on the CPU.

Set comparisons are limited to the outputs guidedmodel.ORDER_FREE names (slots handed out by atomics; equal keys in a tile
sorted by local_sort's network).

NOT COVERED: none -- every wrapper of the header has a probe, a model function and a test (guided_cases.NOT_COVERED is the
list, the host test compares it with the header's declarations).
The giant dictionary of the comparisons is a real one: guidedmodel.derive_giant lays out the distinct phrases longer than
g_depth and sorts their suffixes naively, so cmp_rest's hand-over to it (resolve_small, resolve_medium, batch_lcp) is held
to the plain byte comparison of the alphas.  resolve_small's pair path is run with records that carry ranks and expand = 0,
the only combination the product uses.  bin_hist's 31 / 32 / 33 tiles need texts longer than the others here.

Out of reach of any small input: the launch slicing beyond 2^32 work-items (for_tile_slices, Ctx::tile0 != 0) -- the wrappers
set tile0 themselves -- and stage_block_tiles' lists of 2^32 entries and more.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_cases as C      # noqa: E402
import guidedmodel as GM      # noqa: E402
import kprobe as K            # noqa: E402

pytestmark = pytest.mark.gpu

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
EXTRA = 5


COMPARED = [0]


def compares(count):
    """the test makes exactly `count` comparisons with the model (same(...) calls)"""
    def wrap(fn):
        def run():
            before = COMPARED[0]
            fn()
            assert COMPARED[0] - before == count, (fn.__name__, COMPARED[0] - before)
        run.__name__, run.__doc__ = fn.__name__, fn.__doc__
        return run
    return wrap


def same(got, want, what):
    COMPARED[0] += 1
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not np.array_equal(got, want):
        at = np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8]
        raise AssertionError("%s: differs at %s: got %s, want %s" % (what, at.tolist(), got.reshape(-1)[at].tolist(),
                                                                       want.reshape(-1)[at].tolist()))


# ---- phrase-end tables ---------------------------------------------------------------------------------------------------
def _cut_tables():
    return [(name, GM.CutTables(cuts, n, 5)) for name, (n, cuts) in C.cut_cases().items()]


def test_rank_counts():
    ran = 0
    for name, t in _cut_tables():
        # whole words, and a mask that stops inside a count's eight words (the kernel's `wi < n_words`)
        for n_words in (t.n_words, t.n_words - 3):
            mask = t.mask[:n_words]
            n_counts = (n_words + 7) // 8
            got = K.gk_rank_counts(mask, n_counts, K.sent(n_counts + EXTRA, U32))
            same(got, GM.rank_counts(mask, n_counts, K.sent(n_counts + EXTRA, U32)), name)
            ran += 1
    assert ran == 26


def test_block_first_cut():
    ran = 0
    for name, t in _cut_tables():
        for n_words in (t.n_words, t.n_words - 3):
            mask = t.mask[:n_words]
            got = K.gk_block_first_cut(mask, t.n_blocks, K.sent(t.n_blocks + EXTRA, U64))
            same(got, GM.block_first_cut(mask, t.n_blocks, K.sent(t.n_blocks + EXTRA, U64)), name)
            ran += 1
    assert ran == 26


def test_block_cut_counts():
    ran = 0
    for name, t in _cut_tables():
        for n_words in (t.n_words, t.n_words - 3):
            mask = t.mask[:n_words]
            got = K.gk_block_cut_counts(mask, t.n_blocks, K.sent(t.n_blocks + EXTRA, U32))
            same(got, GM.block_cut_counts(mask, t.n_blocks, K.sent(t.n_blocks + EXTRA, U32)), name)
            ran += 1
    assert ran == 26


def test_block_cut_offsets():
    ran = 0
    for name, t in _cut_tables():
        alloc = len(t.cuts) + EXTRA
        assert C.reject_block_cut_offsets(t.mask, t.brank, t.n_blocks, alloc) is None
        got = K.gk_block_cut_offsets(t.mask, t.brank, t.n_blocks, K.sent(alloc, U16))
        same(got, GM.block_cut_offsets(t.mask, t.brank, t.n_blocks, K.sent(alloc, U16)), name)
        same(got[:len(t.cuts)], t.coff[:len(t.cuts)], name + " (the list layout's table)")
        # blocks laid out with a gap of two entries between them: nothing is written into the gaps
        brank = t.brank[:t.n_blocks] + U32(2) * np.arange(t.n_blocks, dtype=U32)
        alloc = len(t.cuts) + 2 * t.n_blocks + EXTRA
        got = K.gk_block_cut_offsets(t.mask, brank, t.n_blocks, K.sent(alloc, U16))
        same(got, GM.block_cut_offsets(t.mask, brank, t.n_blocks, K.sent(alloc, U16)), name + " (gaps)")
        ran += 2
    assert ran == 26


def test_block_cut_offsets__rejected():
    t = GM.CutTables([1, 2, 3, 5000], 8000, 5)
    assert C.reject_block_cut_offsets(t.mask, t.brank, t.n_blocks, 3) is not None
    with pytest.raises(K.ProbeError, match="beyond coff"):
        K.gk_block_cut_offsets(t.mask, t.brank, t.n_blocks, K.sent(3, U16))


# ---- staged lists (the context-free half) -----------------------------------------------------------------------------------
def _tile_offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(U32), int(np.sum(counts))


STAGE_COUNTS = {
    "one_entry": [1],
    "block_edges": [4095, 1, 1, 4096, 0, 0, 3],            # entries 4095 | 4096 and 8192 | 8193 begin tiles; empty tiles
    "empty_first_tiles": [0, 0, 5000, 0, 4000, 1],
    "many_small": [3] * 3000,                                # a block of the list spans 1366 tiles
    "exact_blocks": [4096, 4096],
}


def test_stage_block_tiles():
    ran = 0
    for name, counts in STAGE_COUNTS.items():
        off, n = _tile_offsets(counts)
        blocks = (n + 4095) // 4096
        got = K.gk_stage_block_tiles(off, n, K.sent(blocks + 1 + EXTRA, U32))
        same(got, GM.stage_block_tiles(off, len(off), n, K.sent(blocks + 1 + EXTRA, U32)), name)
        ran += 1
    got = K.gk_stage_block_tiles(np.zeros(3, U32), 0, K.sent(EXTRA, U32))                   # an empty list: nothing is written
    same(got, K.sent(EXTRA, U32), "empty list")
    assert ran == 5


def test_stage_count():
    rng = np.random.default_rng(21)
    ran = 0
    for n in (1, 15, 16, 4095, 4096, 4097, 3 * 4096 + 17):
        staged = ((rng.integers(0, 40, n) << 12) | rng.integers(0, 4096, n)).astype(U32)
        staged[0] = (4095 << 12) | 4095                                                     # the largest bin of 12 bits
        for b0, b1 in ((0, 4096), (7, 7), (5, 23), (39, 40), (4095, 4096), (0, 1 << 20)):
            blocks = (n + 4095) // 4096
            got = K.gk_stage_count(staged, b0, b1, K.sent(blocks + EXTRA, U32))
            same(got, GM.stage_count(staged, b0, b1, K.sent(blocks + EXTRA, U32)), "n=%d bins [%d, %d)" % (n, b0, b1))
            ran += 1
    same(K.gk_stage_count(np.zeros(0, U32), 0, 9, K.sent(EXTRA, U32)), K.sent(EXTRA, U32), "empty list")
    assert ran == 42


# ---- first keys and rounds --------------------------------------------------------------------------------------------------
def test_heads0():
    ran = 0
    for name, (keys, bits, chars) in C.heads0_cases().items():
        B = len(keys)
        for with_lcp in (True, False):
            mk = lambda: (K.sent(B + EXTRA, U8), K.sent(B + EXTRA, U8), K.sent(B + EXTRA, U32) if with_lcp else None)
            got = K.gk_heads0(keys, bits, chars, *mk())
            want = GM.heads0(keys, bits, chars, *mk())
            same(got[0], want[0], name + " head"); same(got[1], want[1], name + " active")
            if with_lcp:
                same(got[2], want[2], name + " lcp (written at heads j > 0 only)")
            ran += 1
    assert ran == 36


def test_gather_active():
    ran = 0
    for name, (keys, bits, chars) in C.heads0_cases().items():
        B = len(keys)
        head, active, _ = GM.heads0(keys, bits, chars, np.zeros(B, U8), np.zeros(B, U8), None)
        idx = np.flatnonzero(active).astype(U32)
        assert C.reject_index(idx, B, "idx beyond the batch") is None
        pos = (np.arange(B, dtype=U64) << U64(40)) | U64(0xFFFFFFFFFF) - np.arange(B, dtype=U64)     # 64-bit records
        m = len(idx)
        mk = lambda: (K.sent(m + EXTRA, U32), K.sent(m + EXTRA, U64), K.sent(m + EXTRA, U32))
        got = K.gk_gather_active(idx, pos, head, *mk())
        want = GM.gather_active(idx, pos, head, *mk())
        for g, w_, what in zip(got, want, ("slot", "pos", "headval")):
            same(g, w_, name + " " + what)
        ran += 1
    assert ran == 18
    with pytest.raises(K.ProbeError, match="idx beyond the batch"):
        K.gk_gather_active(np.array([0, 4], U32), np.zeros(4, U64), np.zeros(4, U8), K.sent(2, U32), K.sent(2, U64), K.sent(2, U32))


def test_medium_groups():
    ran = 0
    for name, (sizes, cap) in C.medium_cases().items():
        gh = C.gheads(sizes)
        assert C.reject_medium_groups(gh, cap, 4 * cap + 3) is None, name
        lst, cnt = K.gk_medium_groups(gh, cap)
        regions, counts = GM.medium_groups(gh)
        same(cnt, np.array(counts + [K.SENT32], U32), name + " count4")
        for cl in range(4):
            region = lst[cl * cap:(cl + 1) * cap]
            got = sorted((int(a), int(b)) for a, b in region[:counts[cl]])                  # ORDER_FREE inside a region
            assert got == regions[cl], (name, cl, got[:4], regions[cl][:4])
            same(region[counts[cl]:], K.sent(2 * (cap - counts[cl]), U32).reshape(cap - counts[cl], 2), name + " behind region %d" % cl)
        same(lst[4 * cap:], K.sent(6, U32).reshape(-1, 2), name + " behind the list")
        ran += 1
    assert ran == 5


def test_medium_groups__rejected():
    gh = C.gheads([9, 9, 20])
    assert C.reject_medium_groups(gh, 1, 7) is not None
    with pytest.raises(K.ProbeError, match="more groups than a region holds"):
        K.gk_medium_groups(gh, 1)
    with pytest.raises(K.ProbeError, match="names the first of its group"):
        K.gk_medium_groups(np.array([0, 0, 1], U32), 4)


def test_tile_bounds():
    ran = 0
    for name, (sizes, target, limit, n_tiles) in C.bounds_cases().items():
        gh = C.gheads(sizes)
        got = K.gk_tile_bounds(gh, target, limit, n_tiles, K.sent(n_tiles + 1 + EXTRA, U32))
        same(got, GM.tile_bounds(gh, target, limit, n_tiles, K.sent(n_tiles + 1 + EXTRA, U32)), name)
        ran += 1
    # the product's shape: target = half a sort tile, limit = a whole one, 300 tiles (more than a workgroup of the kernel)
    rng = np.random.default_rng(8)
    sizes = [int(s) for s in rng.choice([2, 3, 700, 1100, 2100], 500)]
    gh = C.gheads(sizes)
    n_tiles = (len(gh) + 1023) // 1024
    assert n_tiles > 256
    got = K.gk_tile_bounds(gh, 1024, 2048, n_tiles, K.sent(n_tiles + 1 + EXTRA, U32))
    want = GM.tile_bounds(gh, 1024, 2048, n_tiles, K.sent(n_tiles + 1 + EXTRA, U32))
    assert GM.NO_BOUND in want[:n_tiles].tolist()
    same(got, want, "product shape")
    assert ran == 7


def _check_sorted_tiles(sc, kout, pout, want_k, want_p, network):
    ranges = GM.tile_ranges(sc.bound)
    for b, e in ranges:
        same(kout[b:e], want_k[b:e], "%s keys of tile [%d, %d)" % (sc.name, b, e))       # (sentinels where the tile is big)
        if (b, e) in network:                                                             # ORDER_FREE: equal (group, key)
            gk_sorted = [(int(g), int(k)) for g, k in zip(np.sort(sc.ghead[b:e]), want_k[b:e])]
            assert K.same_sets_per_run(gk_sorted, pout[b:e], want_p[b:e]), "%s records of network tile [%d, %d)" % (sc.name, b, e)
        else:
            same(pout[b:e], want_p[b:e], "%s records of tile [%d, %d)" % (sc.name, b, e))


def test_local_sort():
    ran = networks = 0
    for sc in C.sort_cases():
        assert C.reject_local_sort(sc.ghead, sc.bound, 4, 6) is None, sc.name
        kout, pout, bb, be, cnt = K.gk_local_sort(sc.kin, sc.pin, sc.ghead, sc.bound, K.sent(sc.m, U64), K.sent(sc.m, U64), 6, 4)
        want_k, want_p, big, network = GM.local_sort(sc.kin, sc.pin, sc.ghead, sc.bound, K.sent(sc.m, U64), K.sent(sc.m, U64), 4)
        _check_sorted_tiles(sc, kout, pout, want_k, want_p, network)
        assert cnt == len(big) == sc.n_big, sc.name
        assert sorted(zip(bb[:cnt].tolist(), be[:cnt].tolist())) == big, sc.name           # ORDER_FREE
        same(bb[cnt:], K.sent(6 - cnt, U32), sc.name + " behind big_begin"); same(be[cnt:], K.sent(6 - cnt, U32), sc.name + " behind big_end")
        ran += 1
        networks += len(network)
    assert ran == 4 and networks >= 4


def test_local_sort__big_cap_one_short():
    """two big tiles, room for one: the count still says two, one pair is written, nothing behind the cap"""
    sc = [s for s in C.sort_cases() if s.name == "two_big"][0]
    assert sc.n_big == 2
    kout, pout, bb, be, cnt = K.gk_local_sort(sc.kin, sc.pin, sc.ghead, sc.bound, K.sent(sc.m, U64), K.sent(sc.m, U64), 4, 1)
    want_k, want_p, big, network = GM.local_sort(sc.kin, sc.pin, sc.ghead, sc.bound, K.sent(sc.m, U64), K.sent(sc.m, U64), 1)
    _check_sorted_tiles(sc, kout, pout, want_k, want_p, network)
    assert cnt == 2
    assert (int(bb[0]), int(be[0])) in big
    same(bb[1:], K.sent(3, U32), "behind the cap"); same(be[1:], K.sent(3, U32), "behind the cap")
    kout, pout, bb, be, cnt = K.gk_local_sort(sc.kin, sc.pin, sc.ghead, sc.bound, K.sent(sc.m, U64), K.sent(sc.m, U64), 4, 0)
    assert cnt == 2
    same(bb, K.sent(4, U32), "big_cap = 0")


def test_local_sort__rejected():
    sc = C.sort_cases()[0]
    bad = sc.bound.copy(); bad[1] = 3                                                       # inside the group of 64 at 1
    assert C.reject_local_sort(sc.ghead, bad, 1, 1) is not None
    with pytest.raises(K.ProbeError, match="a bound is a group's head or m"):
        K.gk_local_sort(sc.kin, sc.pin, sc.ghead, bad, K.sent(sc.m, U64), K.sent(sc.m, U64), 1, 1)
    bad = sc.bound.copy(); bad[-1] = GM.NO_BOUND
    with pytest.raises(K.ProbeError, match="the last bound ends every search"):
        K.gk_local_sort(sc.kin, sc.pin, sc.ghead, bad, K.sent(sc.m, U64), K.sent(sc.m, U64), 1, 1)


def test_range_groups():
    ran = 0
    for name, (sizes, ranges) in C.range_cases().items():
        gh = C.gheads(sizes)
        begins, ends = [b for b, _ in ranges], [e for _, e in ranges]
        want = GM.range_groups(gh, begins, ends)
        alloc = len(want) + EXTRA
        assert C.reject_range_groups(gh, begins, ends, alloc) is None, name
        sb, se, cnt = K.gk_range_groups(gh, begins, ends, alloc)
        same(cnt, np.array([len(want), K.SENT32], U32), name + " seg_count")
        assert sorted(zip(sb[:len(want)].tolist(), se[:len(want)].tolist())) == want, name  # ORDER_FREE
        same(sb[len(want):], K.sent(EXTRA, U32), name + " behind seg_begin"); same(se[len(want):], K.sent(EXTRA, U32), name + " behind seg_end")
        ran += 1
    assert ran == 5
    with pytest.raises(K.ProbeError, match="more groups than the segment lists hold"):
        K.gk_range_groups(C.gheads([2, 2, 2]), [0], [6], 2)


def _round_state(seed, m, B):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < m:
        sizes.append(int(rng.choice([1, 1, 2, 3, 9])))
    newhead = C.gheads(sizes)[:m]
    slot = np.sort(rng.choice(B, m, replace=False)).astype(U32)
    pos = rng.integers(0, 1 << 62, m).astype(U64)
    return newhead, slot, pos


def test_round_apply():
    ran = 0
    for seed, m in ((1, 1), (2, 2), (3, 255), (4, 256), (5, 257), (6, 1000)):
        newhead, slot, pos = _round_state(seed, m, 2 * m + 3)
        mk = lambda: (K.sent(2 * m + 3 + EXTRA, U64), K.sent(m + EXTRA, U8))
        got = K.gk_round_apply(pos, newhead, slot, *mk())
        want = GM.round_apply(pos, newhead, slot, *mk())
        same(got[0], want[0], "out m=%d (slots of groups left to the next round stay untouched)" % m)
        same(got[1], want[1], "flags m=%d" % m)
        assert m < 3 or (0 in want[1][:m] and 1 in want[1][:m])
        ran += 1
    assert ran == 6
    with pytest.raises(K.ProbeError, match="slot beyond out"):
        K.gk_round_apply(np.zeros(2, U64), np.array([0, 1], U32), np.array([0, 9], U32), K.sent(9, U64), K.sent(2, U8))


def test_round_compact():
    ran = 0
    for seed, m in ((1, 2), (3, 255), (4, 256), (5, 257), (6, 1000)):
        newhead, slot, pos = _round_state(seed, m, 2 * m + 3)
        _, flags = GM.round_apply(pos, newhead, slot, np.zeros(2 * m + 3, U64), np.zeros(m, U8))
        idx = np.flatnonzero(flags).astype(U32)
        m2 = len(idx)
        mk = lambda: (K.sent(m2 + EXTRA, U32), K.sent(m2 + EXTRA, U64), K.sent(m2 + EXTRA, U32))
        got = K.gk_round_compact(idx, slot, pos, newhead, *mk())
        want = GM.round_compact(idx, slot, pos, newhead, *mk())
        for g, w_, what in zip(got, want, ("slot", "pos", "headval")):
            same(g, w_, "m=%d %s" % (m, what))
        ran += 1
    assert ran == 5
    with pytest.raises(K.ProbeError, match="idx beyond the round's list"):
        K.gk_round_compact(np.array([2], U32), np.zeros(2, U32), np.zeros(2, U64), np.zeros(2, U32), K.sent(1, U32), K.sent(1, U64), K.sent(1, U32))


# ---- giant bookkeeping -------------------------------------------------------------------------------------------------------
SIZES = (1, 31, 32, 33, 255, 256, 257, 1000)


def _parse(seed, m):
    """a parse of m phrases over D distinct ones: (pid, rep, D) with rep[d] = an occurrence of d, not always the first"""
    rng = np.random.default_rng(seed)
    D = max(1, m // 3)
    pid = rng.integers(0, D, m).astype(U32)
    pid[:min(D, m)] = rng.permutation(D)[:min(D, m)]                 # (every distinct phrase occurs when m >= D)
    rep = np.zeros(D, U32)
    for d in range(D):
        occ = np.flatnonzero(pid == d)
        rep[d] = occ[int(rng.integers(0, len(occ)))] if len(occ) else m + 7
    return pid, rep, D


@compares(40)
def test_flag_greater():
    for n in SIZES:
        v = np.random.default_rng(n).integers(0, 50, n).astype(U32)
        v[0] = 0xFFFFFFFF
        for thr in (0, 25, 49, 0xFFFFFFFE, 0xFFFFFFFF):
            same(K.gk_flag_greater(v, thr, K.sent(n + EXTRA, U32)), GM.flag_greater(v, thr, K.sent(n + EXTRA, U32)), "n=%d thr=%d" % (n, thr))


def test_flag_spread():
    ran = 0
    for n in SIZES:
        for k in sorted({0, n // 2, n - 1}):                                                # one flag: at 0, inside, at n - 1
            a = np.zeros(n, U32); a[k] = 4
            same(K.gk_flag_spread(a, K.sent(n + EXTRA, U32)), GM.flag_spread(a, K.sent(n + EXTRA, U32)), "n=%d k=%d" % (n, k))
            ran += 1
        a = np.random.default_rng(n).integers(0, 2, n).astype(U32)
        same(K.gk_flag_spread(a, K.sent(n + EXTRA, U32)), GM.flag_spread(a, K.sent(n + EXTRA, U32)), "n=%d random" % n)
    assert ran == 1 + 7 * 3


@compares(8)
def test_flag_to_distinct():
    for m in SIZES:
        pid, rep, D = _parse(m, m)
        occ = np.random.default_rng(m).integers(0, 3, m).astype(U32) // 2 * 7                # 0 or 7: any non-zero value flags
        got = K.gk_flag_to_distinct(occ, pid, np.concatenate([np.zeros(D, U32), K.sent(EXTRA, U32)]))
        same(got, GM.flag_to_distinct(occ, pid, np.concatenate([np.zeros(D, U32), K.sent(EXTRA, U32)])), "m=%d" % m)
    with pytest.raises(K.ProbeError, match="pid beyond dflag"):
        K.gk_flag_to_distinct(np.ones(2, U32), np.array([0, 5], U32), np.zeros(5, U32))


@compares(8)
def test_flag_from_distinct():
    for m in SIZES:
        pid, rep, D = _parse(m, m)
        dflag = np.random.default_rng(m).integers(0, 2, D).astype(U32) * 3
        same(K.gk_flag_from_distinct(dflag, pid, K.sent(m + EXTRA, U32)), GM.flag_from_distinct(dflag, pid, K.sent(m + EXTRA, U32)), "m=%d" % m)


@compares(8)
def test_flag_scatter_ones():
    for n in SIZES:
        ids = np.random.default_rng(n).choice(2 * n, n, replace=False).astype(U32)
        same(K.gk_flag_scatter_ones(ids, K.sent(2 * n + EXTRA, U32)), GM.flag_scatter_ones(ids, K.sent(2 * n + EXTRA, U32)), "n=%d" % n)
    with pytest.raises(K.ProbeError, match="ids beyond flags"):
        K.gk_flag_scatter_ones(np.array([3], U32), K.sent(3, U32))


@compares(16)
def test_giant_distinct():
    for n in SIZES:
        rng = np.random.default_rng(n)
        D = n + 5
        gids = rng.choice(D, n, replace=False).astype(U32)
        rep = rng.integers(0, 1 << 32, D).astype(U32); dlen = rng.integers(0, 1 << 32, D).astype(U32)
        got = K.gk_giant_distinct(gids, rep, dlen, K.sent(n + EXTRA, U32), K.sent(n + EXTRA, U32))
        want = GM.giant_distinct(gids, rep, dlen, K.sent(n + EXTRA, U32), K.sent(n + EXTRA, U32))
        same(got[0], want[0], "which n=%d" % n); same(got[1], want[1], "glen n=%d" % n)


def test_giant_bits():
    ran = 0
    for m in (1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193):                                 # 8192 flags = 256 words = one workgroup
        flags = np.random.default_rng(m).integers(0, 2, m).astype(U32) * U32(0x80000000)    # non-zero, bit 0 clear
        flags[m - 1] = 1
        words = (m + 31) // 32
        same(K.gk_giant_bits(flags, K.sent(words + EXTRA, U32)), GM.giant_bits(flags, K.sent(words + EXTRA, U32)), "m=%d" % m)
        ran += 1
    assert ran == 10


@compares(8)
def test_popcount_words():
    for n in SIZES:
        bits = np.random.default_rng(n).integers(0, 1 << 32, n).astype(U32)
        bits[0] = 0xFFFFFFFF; bits[-1] = 0 if n > 1 else bits[-1]
        same(K.gk_popcount_words(bits, K.sent(n + EXTRA, U32)), GM.popcount_words(bits, K.sent(n + EXTRA, U32)), "n=%d" % n)


@compares(8)
def test_giant_map():
    for n in SIZES:
        rng = np.random.default_rng(n)
        gids = rng.choice(3 * n, n, replace=False).astype(U32); gstart = rng.integers(0, 1 << 32, n).astype(U32)
        same(K.gk_giant_map(gids, gstart, K.sent(3 * n + EXTRA, U32)), GM.giant_map(gids, gstart, K.sent(3 * n + EXTRA, U32)), "n=%d" % n)
    with pytest.raises(K.ProbeError, match="gids beyond dmap"):
        K.gk_giant_map(np.array([4], U32), np.array([1], U32), K.sent(4, U32))


def test_giant_occurrences():
    ran = 0
    for m in SIZES:
        for wide in (False, True):
            pid, rep, D = _parse(m + 100, m)
            rng = np.random.default_rng(m)
            pstart = np.sort(rng.integers(0, 1 << 32, m)).astype(U64)
            if wide:
                pstart = pstart + (U64(1) << U64(32)) * np.arange(m, dtype=U64)              # starts above 2^32: no text is read
                assert int(pstart[-1]) >= 1 << 32 or m == 1
            gk = np.flatnonzero(rng.integers(0, 2, m)).astype(U32)
            gk = gk if len(gk) else np.array([m - 1], U32)
            dmap = rng.integers(0, 1 << 32, D).astype(U32)
            n = len(gk)
            got = K.gk_giant_occurrences(gk, pid, pstart, wide, dmap, K.sent(n + EXTRA, U64), K.sent(n + EXTRA, U32))
            want = GM.giant_occurrences(gk, pid, pstart, dmap, K.sent(n + EXTRA, U64), K.sent(n + EXTRA, U32))
            same(got[0], want[0], "gps m=%d wide=%d" % (m, wide)); same(got[1], want[1], "gbase m=%d wide=%d" % (m, wide))
            ran += 1
    assert ran == 16
    with pytest.raises(K.ProbeError, match="gk beyond the parse"):
        K.gk_giant_occurrences(np.array([2], U32), np.zeros(2, U32), np.zeros(2, U32), False, np.zeros(1, U32), K.sent(1, U64), K.sent(1, U32))


@compares(8)
def test_giant_group_flags():
    for nd in SIZES:
        rng = np.random.default_rng(nd)
        ln = rng.integers(1, 4, nd).astype(U32)
        esuf = ln | (rng.integers(0, 2, nd).astype(U32) << U32(31))                          # the top bit is not part of the length
        lcp = (ln.astype(np.int64) + rng.integers(-1, 2, nd)).astype(U32)                    # length - 1, length, length + 1
        same(K.gk_giant_group_flags(esuf, lcp, K.sent(nd + EXTRA, U32)), GM.giant_group_flags(esuf, lcp, K.sent(nd + EXTRA, U32)), "nd=%d" % nd)


# ---- results (the context-free half) ---------------------------------------------------------------------------------------
@compares(9)
def test_group_ids():
    for B in SIZES:
        rng = np.random.default_rng(B)
        flags = rng.integers(0, 2, B).astype(U32)
        gscan = np.cumsum(flags).astype(U32)
        mk = lambda: np.concatenate([flags, K.sent(EXTRA, U32)])
        same(K.gk_group_ids(mk(), gscan, B), GM.group_ids(mk(), gscan, B), "B=%d" % B)
    same(K.gk_group_ids(K.sent(EXTRA, U32), np.zeros(0, U32), 0), K.sent(EXTRA, U32), "B=0")


def test_add_offset():
    ran = 0
    for n in SIZES:
        for dtype, add in ((U32, 12345), (U32, 0xFFFFFFFF), (U64, 12345), (U64, (1 << 40) + 3), (U64, (1 << 63) + 1)):
            a = np.concatenate([np.random.default_rng(n).integers(0, 1 << 32, n).astype(dtype), K.sent(EXTRA, dtype)])
            a[0] = np.iinfo(dtype).max                                                       # wraps in the table's own width
            same(K.gk_add_offset(a.copy(), n, add), GM.add_offset(a.copy(), n, add), "n=%d %s add=%d" % (n, dtype.__name__, add))
            ran += 1
    same(K.gk_add_offset(K.sent(EXTRA, U64), 0, 5), K.sent(EXTRA, U64), "n=0")
    assert ran == 40


def test_rep_bits():
    ran = 0
    for m in (1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193):
        pid, rep, D = _parse(m, m)
        words = (m + 31) // 32
        same(K.gk_rep_bits(pid, rep, K.sent(words + EXTRA, U32)), GM.rep_bits(pid, rep, K.sent(words + EXTRA, U32)), "m=%d" % m)
        ran += 1
    assert ran == 10
    with pytest.raises(K.ProbeError, match="pid beyond rep"):
        K.gk_rep_bits(np.array([1], U32), np.zeros(1, U32), K.sent(1, U32))


# ==== the wrappers that read gk::Ctx ===============================================================================================
TEXTS = C.text_cases()
LAYOUTS = ("bytes", "packed")
HALF = GM.RUN_BUCKETS_HALF


def _tile_offsets_of(counts, gap=0):
    """exclusive sums of per-tile counts, `gap` unused entries between tiles (nothing may be written there)"""
    off, at = [], 0
    for c_ in counts:
        off.append(at)
        at += int(c_) + gap
    return np.array(off, dtype=U32), at


def test_tile_lead():
    ran = 0
    for name, text in TEXTS.items():
        c = C.make_ctx(text)
        for layout in LAYOUTS:
            mk = lambda: (K.sent(c.tiles + EXTRA, U8), K.sent(c.tiles + EXTRA, U16), K.sent(c.tiles + EXTRA, U8))
            got = K.gk_tile_lead(K.GkCtx(c, layout), *mk())
            want = GM.tile_lead(c, *mk())
            for g, w_, what in zip(got, want, ("first", "lead", "follow")):
                same(g, w_, "%s %s %s" % (name, layout, what))
            ran += 1
    assert ran == 2 * len(TEXTS) == 32


def _hist_forms(name):
    """(text layout, phrase-end layout, rep, no_dense) of a text: every text in both text layouts; the expansion's filter in both
    phrase-end layouts on a few"""
    forms = [("bytes", "bits", None, 0), ("packed", "bits", None, 0), ("packed", "bits", None, 1)]
    if name in ("n=3x4096+1", "exception@4096", "runs", "plain64"):
        forms += [(tl, cl, rep, 0) for tl in LAYOUTS for cl in ("bits", "list") for rep in ("all", "alternate")]
    return forms


def test_bin_hist():
    ran = dense_and_staged = 0
    for name, text in TEXTS.items():
        for tl, cl, rep, nd in _hist_forms(name):
            c = C.make_ctx(text, rep=rep)
            g = K.GkCtx(c, tl, cl, nd)
            d = GM.dense_tiles(c, tl, nd)
            dense_and_staged += 0 < len(d) < c.tiles
            for pc in (1, 4):
                nb = 1 << (c.bits * pc)
                mk = lambda: np.concatenate([np.zeros(nb, U64), K.sent(EXTRA, U64)])
                same(K.gk_bin_hist(g, pc, mk()), GM.bin_hist(c, pc, mk()), "%s %s %s rep=%s no_dense=%d pc=%d" % (name, tl, cl, rep, nd, pc))
                ran += 1
    assert ran == 2 * (3 * 16 + 8 * 4) and dense_and_staged >= 8       # a dense and a staged tile in one launch


def test_bin_hist__31_32_33_tiles():
    """a workgroup counts 32 tiles before its counters leave: texts of 31, 32 and 33 tiles (longer than any other text here:
    the loop has no smaller edge); the histogram is the sum of batch_count over a partition of the bins"""
    rng = np.random.default_rng(9)
    for tiles in (31, 32, 33):
        text = C._bases(rng, tiles * 4096 + 70)
        text[40000:40040] = ord("N")
        c = C.make_ctx(text)
        for tl in LAYOUTS:
            g = K.GkCtx(c, tl)
            hist = K.gk_bin_hist(g, 4, np.zeros(4096, U64))
            same(hist, GM.bin_hist(c, 4, np.zeros(4096, U64)), "%d tiles %s" % (tiles, tl))
            total = np.zeros(c.tiles, np.int64)
            for lo, hi in ((0, 1500), (1500, 1501), (1501, 4096)):
                cnt = K.gk_batch_count(g, 4, lo, hi, K.sent(c.tiles + EXTRA, U32))
                same(cnt, GM.batch_count(c, 4, lo, hi, K.sent(c.tiles + EXTRA, U32)), "%d tiles %s bins [%d, %d)" % (tiles, tl, lo, hi))
                assert int(cnt[:c.tiles].sum()) == int(hist[lo:hi].sum())
                total += cnt[:c.tiles]
            assert total.tolist() == [min(4096, c.n - 4096 * t) for t in range(c.tiles)]


def test_batch_count():
    ran = 0
    for name, text in TEXTS.items():
        for tl, cl, rep, nd in _hist_forms(name):
            c = C.make_ctx(text, rep=rep)
            g = K.GkCtx(c, tl, cl, nd)
            for pc in (1, 4):
                for lo, hi in C.bin_ranges(c, pc):
                    got = K.gk_batch_count(g, pc, lo, hi, K.sent(c.tiles + EXTRA, U32))
                    same(got, GM.batch_count(c, pc, lo, hi, K.sent(c.tiles + EXTRA, U32)),
                         "%s %s %s rep=%s no_dense=%d pc=%d bins [%d, %d)" % (name, tl, cl, rep, nd, pc, lo, hi))
                    ran += 1
    assert ran == 2 * 6 * (3 * 16 + 8 * 4)


def _fill_forms(name):
    forms = [("bytes", "bits", None, "len"), ("packed", "bits", None, "len"), ("packed", "list", None, "rank")]
    if name in ("n=3x4096+1", "exception@4096", "runs", "plain64"):
        forms += [("packed", cl, rep, "len") for cl in ("bits", "list") for rep in ("all", "alternate")] + [("bytes", "list", "alternate", "rank")]
    return forms


def test_batch_fill():
    """keys, records and order against the model; per-tile offsets with a gap of three entries between tiles (untouched);
    next_count present and null"""
    ran = dense_and_staged = 0
    for name, text in TEXTS.items():
        for tl, cl, rep, rec in _fill_forms(name):
            c = C.make_ctx(text, rep=rep, rec=rec)
            g = K.GkCtx(c, tl, cl)
            dense_and_staged += 0 < len(GM.dense_tiles(c, tl)) < c.tiles
            pc = 4
            ranges = C.bin_ranges(c, pc)
            for i, (lo, hi) in enumerate(ranges):
                nlo, nhi = ranges[(i + 1) % len(ranges)]
                counts = GM.batch_count(c, pc, lo, hi, np.zeros(c.tiles, U32))
                off, total = _tile_offsets_of(counts, gap=3)
                with_next = i % 2 == 0
                mk = lambda: (K.sent(total + 4096 + EXTRA, U64), K.sent(total + 4096 + EXTRA, U64), K.sent(c.tiles + EXTRA, U32) if with_next else None)
                got = K.gk_batch_fill(g, pc, lo, hi, off, *mk()[:2], nlo, nhi, mk()[2])
                want = GM.batch_fill(c, pc, lo, hi, off, *mk()[:2], nlo, nhi, mk()[2])
                what = "%s %s %s rep=%s rec=%s bins [%d, %d)" % (name, tl, cl, rep, rec, lo, hi)
                same(got[0], want[0], what + " keys"); same(got[1], want[1], what + " records")
                if with_next:
                    same(got[2], want[2], what + " next_count")
                ran += 1
    assert ran == 6 * (3 * 16 + 5 * 4) and dense_and_staged >= 8


def test_stage_fill():
    ran = 0
    for name, text in TEXTS.items():
        for tl, cl, rep, rec in _fill_forms(name):
            c = C.make_ctx(text, rep=rep, rec=rec)
            g = K.GkCtx(c, tl, cl)
            pc = 4
            for lo, hi, nlo, nhi in ((0, 4096, 7, 7), (1755, 3300, 0, 1755)):
                counts = GM.batch_count(c, pc, lo, hi, np.zeros(c.tiles, U32))
                off, total = _tile_offsets_of(counts, gap=2)
                mk = lambda: (K.sent(total + 4096 + EXTRA, U32), K.sent(c.tiles + EXTRA, U32))
                got = K.gk_stage_fill(g, pc, lo, hi, off, mk()[0], nlo, nhi, mk()[1])
                want = GM.stage_fill(c, pc, lo, hi, off, mk()[0], nlo, nhi, mk()[1])
                what = "%s %s %s rep=%s bins [%d, %d)" % (name, tl, cl, rep, lo, hi)
                same(got[0], want[0], what + " staged"); same(got[1], want[1], what + " next_count")
                ran += 1
    assert ran == 2 * (3 * 16 + 5 * 4)


def test_stage_take():
    """a pass staged by the MODEL, then every batch of it taken by the kernel: the same keys, records and order as batch_fill's
    model gives for that batch, block offsets with a gap (untouched); the next batch's counts present and null"""
    ran = 0
    for name, text in TEXTS.items():
        for tl, cl, rep, rec in _fill_forms(name)[:4]:
            c = C.make_ctx(text, rep=rep, rec=rec)
            g = K.GkCtx(c, tl, cl)
            pc, lo, hi = 4, 1000, 4096
            counts = GM.batch_count(c, pc, lo, hi, np.zeros(c.tiles, U32))
            off, n = _tile_offsets_of(counts)
            if n == 0:
                continue
            staged, _ = GM.stage_fill(c, pc, lo, hi, off, np.zeros(n, U32), 0, 0, None)
            blocks = (n + 4095) // 4096
            blk_tile = GM.stage_block_tiles(off, c.tiles, n, np.zeros(blocks + 1, U32))
            for b0, b1, nb0, nb1 in ((1000, 2400, 2400, 4096), (2400, 4096, 0, 0), (1755, 1756, 1000, 1001)):
                per_block = GM.stage_count(staged, b0, b1, np.zeros(blocks, U32))
                boff, total = _tile_offsets_of(per_block, gap=2)
                with_next = nb1 > nb0
                mk = lambda: (K.sent(total + 4096 + EXTRA, U64), K.sent(total + 4096 + EXTRA, U64), K.sent(blocks + EXTRA, U32) if with_next else None)
                got = K.gk_stage_take(g, staged, b0, b1, boff, *mk()[:2], nb0, nb1, mk()[2], off, blk_tile)
                want = GM.stage_take(c, staged, b0, b1, boff, *mk()[:2], nb0, nb1, mk()[2], off)
                what = "%s %s %s rec=%s bins [%d, %d)" % (name, tl, cl, rec, b0, b1)
                same(got[0], want[0], what + " keys"); same(got[1], want[1], what + " records")
                if with_next:
                    same(got[2], want[2], what + " next_count")
                # ... which is what batch_fill yields for the batch: the same keys and records in the same order
                bcounts = GM.batch_count(c, pc, b0, b1, np.zeros(c.tiles, U32))
                toff, btotal = _tile_offsets_of(bcounts)
                fk, fp, _ = GM.batch_fill(c, pc, b0, b1, toff, np.zeros(btotal, U64), np.zeros(btotal, U64), 0, 0, None)
                taken_k = np.concatenate([got[0][int(o):int(o) + int(k)] for o, k in zip(boff, per_block)])
                taken_p = np.concatenate([got[1][int(o):int(o) + int(k)] for o, k in zip(boff, per_block)])
                same(taken_k, fk, what + " keys as batch_fill"); same(taken_p, fp, what + " records as batch_fill")
                ran += 1
    assert ran == 3 * (3 * 12 + 4 * 4)


def _run_tables(c, sym, extra_lead=None):
    first, lead, follow = GM.tile_lead(c, np.zeros(c.tiles, U8), np.zeros(c.tiles, U16), np.zeros(c.tiles, U8))
    if extra_lead is not None:                      # a forged entry for the tile behind the last: the run goes on for that long
        first = np.append(first, U8(sym)); lead = np.append(lead, U16(0)); follow = np.append(follow, U8(extra_lead[1]))
    whole, fol = GM.chain_leads(first, lead, follow, len(first))
    if extra_lead is not None:
        whole[-1] = extra_lead[0]
    return first, whole, fol


SLICES = ((0, 2 * HALF), (0, 256), (256, HALF), (0, HALF), (HALF, 2 * HALF), (300, 300), (2 * HALF - 256, 2 * HALF - 255))


def test_run_hist():
    ran = 0
    for name, letter in (("runs", "T"), ("runs", "N"), ("long_runs", "T"), ("n_run_3_tiles", "N")):
        for rep in (None, "alternate"):
            c = C.make_ctx(TEXTS[name], rep=rep)
            sym = int(c.code[ord(letter)])
            first, whole, fol = _run_tables(c, sym)
            rs = GM.RunSlice(sym, 5, 6, whole, first, fol)                    # (the slice's own range is not looked at)
            for tl, pc in (("bytes", 1), ("packed", 4)):
                bin_ = sum(sym << (c.bits * i) for i in range(pc))
                mk = lambda: np.concatenate([np.zeros(4 * HALF, U64), K.sent(EXTRA, U64)])
                got = K.gk_run_hist(K.GkCtx(c, tl, "list" if rep else "bits"), pc, bin_, rs, mk())
                want = GM.run_hist(c, pc, bin_, rs, mk())
                same(got, want, "%s %s rep=%s %s pc=%d" % (name, letter, rep, tl, pc))
                assert int(want[:2 * HALF].sum()) > 30
                ran += 1
    assert ran == 16


def test_batch_count__run_slices():
    """slices of the run bin: by bucket ranges that cut at 255 | 256 and at HALF - 1 | HALF, an empty one; the counts of the
    slices of a partition add up to the bin"""
    ran = 0
    for name, letter in (("runs", "T"), ("runs", "N"), ("long_runs", "T"), ("n_run_3_tiles", "N")):
        c = C.make_ctx(TEXTS[name])
        sym = int(c.code[ord(letter)])
        first, whole, fol = _run_tables(c, sym)
        pc = 4
        bin_ = sum(sym << (c.bits * i) for i in range(pc))
        for tl in LAYOUTS:
            g = K.GkCtx(c, tl)
            for blo, bhi in SLICES:
                rs = GM.RunSlice(sym, blo, bhi, whole, first, fol)
                got = K.gk_batch_count(g, pc, bin_, bin_ + 1, K.sent(c.tiles + EXTRA, U32), rs)
                same(got, GM.batch_count(c, pc, bin_, bin_ + 1, K.sent(c.tiles + EXTRA, U32), rs), "%s %s %s buckets [%d, %d)" % (name, letter, tl, blo, bhi))
                ran += 1
        whole_bin = GM.batch_count(c, pc, bin_, bin_ + 1, np.zeros(c.tiles, U32))
        parts = [GM.batch_count(c, pc, bin_, bin_ + 1, np.zeros(c.tiles, U32), GM.RunSlice(sym, a, b, whole, first, fol)) for a, b in ((0, 256), (256, HALF), (HALF, 2 * HALF))]
        assert np.array_equal(sum(p.astype(np.int64) for p in parts), whole_bin)
    assert ran == 4 * 2 * 7


FORGED_R = (2 ** 8, 2 ** 9, 2 ** 32, 2 ** 40 - 1, 2 ** 40 + 5)


def test_batch_fill__run_slices_and_forged_leads():
    """a text that ends, at a tile's end, in ten T: a forged table entry for the tile behind it lets the run go on, so that
    r = 2^8 +- 1, 2^9, 2^32 +- 1, 2^40 - 1 and 2^40 + 5 reach run_bucket; followed by a symbol below and above T"""
    rng = np.random.default_rng(3)
    text = C._bases(rng, 2 * 4096, b"ACG")
    text[-10:] = ord("T")
    text[100:400] = ord("T")
    c = C.make_ctx(text)
    sym = int(c.code[ord("T")])
    pc = 4
    bin_ = sum(sym << (c.bits * i) for i in range(pc))
    ran = 0
    seen = set()
    for R in FORGED_R:
        for follow in (1, 0):                                   # the Dollar (below T); nothing at all (reads 0: below)
            first, whole, fol = _run_tables(c, sym, (R - 5, follow))
            for blo, bhi in ((0, 2 * HALF), (0, HALF), (HALF, 2 * HALF), (GM.run_bucket(R, True), GM.run_bucket(R, True) + 1)):
                rs = GM.RunSlice(sym, blo, bhi, whole, first, fol)
                seen |= {GM.run_at(c, rs, p)[0] for p in range(c.n - 10, c.n)}
                counts = GM.batch_count(c, pc, bin_, bin_ + 1, np.zeros(c.tiles, U32), rs)
                for tl in LAYOUTS:
                    g = K.GkCtx(c, tl)
                    same(K.gk_batch_count(g, pc, bin_, bin_ + 1, K.sent(c.tiles + EXTRA, U32), rs),
                         GM.batch_count(c, pc, bin_, bin_ + 1, K.sent(c.tiles + EXTRA, U32), rs), "R=%d count" % R)
                    off, total = _tile_offsets_of(counts, gap=1)
                    mk = lambda: (K.sent(total + 4096 + EXTRA, U64), K.sent(total + 4096 + EXTRA, U64))
                    got = K.gk_batch_fill(g, pc, bin_, bin_ + 1, off, *mk(), 0, 0, None, rs)
                    want = GM.batch_fill(c, pc, bin_, bin_ + 1, off, *mk(), 0, 0, None, rs)
                    same(got[0], want[0], "R=%d keys" % R); same(got[1], want[1], "R=%d records" % R)
                    ran += 1
    assert ran == 5 * 2 * 4 * 2
    for R in (2 ** 8 - 1, 2 ** 8 + 1, 2 ** 9, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 40 - 1, 2 ** 40 + 5):
        assert R in seen, R


def test_phrase_items():
    ran = 0
    for name in ("n=1x4096+1", "exception@4096", "runs"):
        for wide in (False, True):
            for tl in LAYOUTS:
                c = C.make_ctx(TEXTS[name], skip=1)
                pstart = [c.phrase_start(k) for k in range(c.m)]
                rep = np.random.default_rng(5).permutation(c.m)[:c.m // 2 + 1]
                mk = lambda: (K.sent(len(rep) + EXTRA, U64), K.sent(len(rep) + EXTRA, U64))
                got = K.gk_phrase_items(K.GkCtx(c, tl, "list" if wide else "bits"), pstart, wide, rep, *mk())
                want = GM.phrase_items(c, pstart, rep, *mk())
                same(got[0], want[0], "%s keys" % name); same(got[1], want[1], "%s records" % name)
                assert all((int(r) >> 40) == c.phrase_len(int(k)) for r, k in zip(want[1], rep))      # a phrase's alpha is the phrase
                ran += 1
    assert ran == 12


def _giant_ctx(name, **kw):
    c = C.make_ctx(TEXTS[name], g_depth=42, **kw)
    c.giant = C.real_giant(c)
    assert 3 <= sum(c.giant.flag) < sum(1 for k in range(c.m) if c.phrase_len(k) > 42)
    return c


def _elements(c, offset, seed, count=500):
    """V indices: a random sample, every suffix whose alpha is spent exactly at `offset` or one character later, the first and
    the last text position"""
    rng = np.random.default_rng(seed)
    q = set(int(x) for x in rng.integers(1, c.n + 1, count)) | {1, c.n}
    q |= {x for x in range(1, c.n + 1, 1) if c.alpha_len(x) in (offset, offset + 1)} if offset else set()
    return sorted(q)


def _records(c, qs, form):
    assert C.reject_elements(c, qs) is None
    if form == "sat":                                       # a length field forged to LEN_SAT over a short alpha: looked up again
        return np.array([q | (GM.LEN_SAT << 40) for q in qs], dtype=U64)
    return np.array([c.make_rec(q) for q in qs], dtype=U64)


def test_round_keys():
    ran = 0
    counts = {"spent": 0, "giant": 0, "chars": 0}
    for name in ("exception@4096", "runs"):
        for form in ("len", "rank", "sat"):
            c = _giant_ctx(name, rec="rank" if form == "rank" else "len")
            for tl, cl in (("bytes", "bits"), ("packed", "list")):
                g = K.GkCtx(c, tl, cl)
                for offset in (0, 6, 21, 42, 63, 700):
                    pos = _records(c, _elements(c, offset, offset), form)
                    m = len(pos)
                    mk = lambda: (K.sent(m + EXTRA, U64), np.concatenate([np.zeros(3, U32), K.sent(13, U32)]))
                    got = K.gk_round_keys(g, pos, offset, *mk())
                    want = GM.round_keys(c, pos, offset, *mk())
                    what = "%s %s %s %s offset=%d" % (name, form, tl, cl, offset)
                    same(got[0], want[0], what + " keys"); same(got[1], want[1], what + " err")
                    for k in want[0][:m]:
                        counts["spent" if int(k) >> 63 else ("giant" if offset >= 42 and (int(k) >> 32) == (GM.GIANT_KEY >> 32) else "chars")] += 1
                    ran += 1
    assert ran == 2 * 3 * 2 * 6 and min(counts.values()) > 500, counts


def test_round_keys__phrases():
    """skip = 1: an element whose phrase is spent is a duplicate distinct phrase: err[0] counts it, its key is its own index"""
    c = C.make_ctx(TEXTS["runs"], skip=1)
    starts = [c.phrase_start(k) for k in range(c.m)]
    pos = _records(c, starts + starts[3:5], "len")              # (a forged duplicate changes nothing for the kernel: offsets do)
    g = K.GkCtx(c, "packed", "bits")
    ran = 0
    for offset in (0, 21, 63, 126):
        mk = lambda: (K.sent(len(pos) + EXTRA, U64), np.concatenate([np.zeros(3, U32), K.sent(13, U32)]))
        got = K.gk_round_keys(g, pos, offset, *mk())
        want = GM.round_keys(c, pos, offset, *mk())
        same(got[0], want[0], "offset=%d keys" % offset); same(got[1], want[1], "offset=%d err" % offset)
        ran += int(want[1][0]) > 0
    assert ran >= 2


def _probe_groups(c, offset, seed):
    """elements grouped so that some groups are pure (every member inside a giant occurrence, alpha unspent), some hold a
    member outside, some a member whose alpha is spent"""
    inside = [q for q in range(1, c.n + 1) if c.giant_entry(q, 0) is not None and c.alpha_len(q) > offset]
    spent = [q for q in range(1, c.n + 1) if c.giant_entry(q, 0) is not None and c.alpha_len(q) <= offset]
    outside = [q for q in range(1, c.n + 1, 7) if c.giant_entry(q, 0) is None and c.alpha_len(q) > offset]
    rng = np.random.default_rng(seed)
    qs, sizes = [], []
    for kind in range(60):
        size = int(rng.integers(1, 6))
        members = [inside[int(i)] for i in rng.integers(0, len(inside), size)]
        if kind % 3 == 1:
            members[int(rng.integers(0, size))] = outside[int(rng.integers(0, len(outside)))]
        if kind % 3 == 2 and spent:
            members[int(rng.integers(0, size))] = spent[int(rng.integers(0, len(spent)))]
        qs += members; sizes.append(size)
    return qs, C.gheads(sizes)


def test_giant_probe():
    ran = 0
    for form in ("len", "rank"):
        c = _giant_ctx("runs", rec=form, expand=0 if form == "rank" else 1)
        for tl, cl in (("bytes", "list"), ("packed", "bits")):
            g = K.GkCtx(c, tl, cl)
            for offset in (0, 21, 50):
                qs, ghead = _probe_groups(c, offset, offset)
                pos = _records(c, qs, form)
                m = len(pos)
                mk = lambda: (K.sent(m + EXTRA, U32), K.sent(m + EXTRA, U8))
                got = K.gk_giant_probe(g, pos, ghead, offset, *mk())
                want = GM.giant_probe(c, pos, ghead, offset, *mk())
                same(got[0], want[0], "%s offset=%d gr" % (form, offset)); same(got[1], want[1], "%s offset=%d pure" % (form, offset))
                heads = sorted(set(ghead.tolist()))
                assert 10 <= sum(int(want[1][h]) for h in heads) <= len(heads) - 20           # pure groups and cleared ones
                # ... and round_keys hands the pure groups their entries
                mk2 = lambda: (K.sent(m + EXTRA, U64), np.concatenate([np.zeros(3, U32), K.sent(13, U32)]))
                gotk = K.gk_round_keys(g, pos, offset, *mk2(), want[0][:m], want[1][:m], ghead)
                wantk = GM.round_keys(c, pos, offset, *mk2(), want[0][:m], want[1][:m], ghead)
                same(gotk[0], wantk[0], "%s offset=%d keys of pure groups" % (form, offset)); same(gotk[1], wantk[1], "err")
                ran += 1
    assert ran == 12


def _heads_input(c, seed, with_pure):
    """keys of a round, sorted inside the old groups: characters (some with bit 62 set and bits 32 .. 61 clear: 21 symbols of
    three bits whose first is C and whose next ten are padding), ranks, entries of the giant dictionary; a group that mixes
    spent and unspent keys"""
    rng = np.random.default_rng(seed)
    size = len(c.giant.isa)
    grp = c.giant.grp
    twins = [r for r in range(size - 1) if int(grp[r]) == int(grp[r + 1])]       # two entries of one group of equal strings
    assert len(twins) > 100
    keys, sizes, pure = [], [], []
    for gi in range(80):
        n_el = int(rng.integers(1, 9))
        kind = gi % 5
        if kind == 0:        # characters: near keys, so that neighbours share many symbols
            base = int(rng.integers(0, 1 << 62))
            ks = [base ^ (1 << int(rng.integers(0, 63))) if rng.integers(0, 2) else base for _ in range(n_el)]
        elif kind == 1:      # characters that look like giant keys
            ks = [GM.GIANT_KEY | int(rng.integers(0, min(size, 1 << 20))) for _ in range(n_el)]
        elif kind == 2:      # ranks
            ks = [GM.RANK_KEY | int(x) for x in rng.choice(1 << 20, n_el, replace=False)]
        elif kind == 3:      # entries of the giant dictionary: two of one group of equal strings, one of them twice, and others
            r = twins[int(rng.integers(0, len(twins)))]
            ks = [GM.GIANT_KEY | x for x in [r, r + 1, r + 1] + [int(rng.integers(0, size)) for _ in range(n_el)]]
        else:                # spent and unspent in one group (not prefix-free: err[1])
            ks = [int(rng.integers(0, 1 << 62)) for _ in range(n_el)] + [GM.RANK_KEY | 5]
        ks.sort()
        keys += ks; sizes.append(len(ks))
        pure += [1 if with_pure and kind in (1, 3) and gi % 2 else 0] * len(ks)
    return np.array(keys, dtype=U64), C.gheads(sizes), np.array(pure, dtype=U8)


def _giant_pairs(c, keys, ghead, pure, offset):
    """from the input alone: the places whose key and the key before it, inside one old group, are read as entries of the giant
    dictionary (a round beyond g_depth, or a pure group) -- (of two groups of equal strings, of one group with two entries, the
    same entry twice)"""
    two, one, twice = [], [], []
    for e in range(1, len(keys)):
        g0 = int(ghead[e])
        if g0 == e or not (offset >= c.g_depth or (pure is not None and pure[g0])):
            continue
        k, kp = int(keys[e]), int(keys[e - 1])
        if (k >> 32) == (GM.GIANT_KEY >> 32) and (kp >> 32) == (GM.GIANT_KEY >> 32):
            r, rp = k & 0xFFFFFFFF, kp & 0xFFFFFFFF
            (twice if r == rp else one if int(c.giant.grp[r]) == int(c.giant.grp[rp]) else two).append(e)
    return two, one, twice


def test_round_heads():
    ran = hinted = bit62_as_chars = 0
    heads_of = {}
    for expand in (0, 1):
        c = _giant_ctx("runs", expand=expand)
        g = K.GkCtx(c, "bytes", "bits")
        for offset, with_pure in ((21, False), (21, True), (42, False), (84, True)):          # g_depth = 42: the last two are giant rounds
            keys, ghead, pure = _heads_input(c, offset, with_pure)          # (the same input for both values of expand)
            m = len(keys)
            two, one, twice = _giant_pairs(c, keys, ghead, pure if with_pure else None, offset)
            assert (len(two) > 20 and len(one) >= 8 and len(twice) >= 8) if (offset >= 42 or with_pure) else not (two or one or twice)
            slot = np.random.default_rng(1).permutation(2 * m)[:m].astype(U32)
            for with_lcp in (True, False):
                mk = lambda: (K.sent(m + EXTRA, U32), np.concatenate([np.zeros(3, U32), K.sent(13, U32)]), K.sent(2 * m + EXTRA, U32) if with_lcp else None)
                args = (slot if with_lcp else None, offset, pure if with_pure else None)
                got = K.gk_round_heads(g, keys, ghead, *mk(), *args)
                want = GM.round_heads(c, keys, ghead, *mk(), *args)
                what = "expand=%d offset=%d pure=%d lcp=%d" % (expand, offset, with_pure, with_lcp)
                same(got[0], want[0], what + " headval"); same(got[1], want[1], what + " err")
                assert int(want[1][1]) > 0
                # entries of one group of equal strings stay together until the parse ranks decide -- but representatives
                # (expand) part at once: the two runs differ exactly there
                for e in one + twice:
                    assert int(want[0][e]) == (e if expand else 0), (what, e)
                for e in two:
                    assert int(want[0][e]) == e, (what, e)
                if expand:
                    assert np.flatnonzero(want[0] != heads_of[(offset, with_pure, with_lcp)]).tolist() == sorted(one + twice), what
                else:
                    heads_of[(offset, with_pure, with_lcp)] = want[0]
                if with_lcp:
                    same(got[2], want[2], what + " lcp_out (written only where the model says)")
                    hinted += int((want[2] != U32(K.SENT32)).sum())
                    if offset < 42:
                        for e in range(1, m):
                            if (int(keys[e]) >> 32) == (GM.GIANT_KEY >> 32) and ghead[e] != e and keys[e] != keys[e - 1] and not (with_pure and pure[ghead[e]]):
                                bit62_as_chars += int(want[2][slot[e]]) == offset + GM.common_symbols(keys[e], keys[e - 1], c.bits, c.chars)
                ran += 1
    assert ran == 16 and hinted > 200 and bit62_as_chars > 10


def test_write_columns():
    ran = 0
    for name in ("n=1x4096+1", "exception@4096"):
        for form in ("len", "rank"):
            c = C.make_ctx(TEXTS[name], rec=form)
            for tl in LAYOUTS:
                g = K.GkCtx(c, tl)
                pos = _records(c, _elements(c, 0, 3, 300), form)
                B = len(pos)
                for base, wide in ((0, False), (7, False), (7, True)):
                    mk = lambda: (K.sent(base + B + EXTRA, U32), K.sent(base + B + EXTRA, U8) if wide else None, K.sent(base + B + EXTRA, U8))
                    got = K.gk_write_columns(g, pos, base, *mk())
                    want = GM.write_columns(c, pos, base, *mk())
                    what = "%s %s %s base=%d wide=%d" % (name, form, tl, base, wide)
                    same(got[0], want[0], what + " sa"); same(got[2], want[2], what + " bwt")
                    if wide:
                        same(got[1], want[1], what + " sa high bytes")
                    assert int(want[2][base]) == 0 and c.rec_pos(pos[0]) == 1                   # q = 1: the BWT reads 0
                    ran += 1
    assert ran == 24


def test_phrase_ranks():
    ran = 0
    for name in ("n=3x4096+1", "runs"):
        for tl, cl in (("bytes", "bits"), ("packed", "list")):
            c = C.make_ctx(TEXTS[name], skip=1)
            order = np.random.default_rng(4).permutation(c.m)                                   # any order of the phrases: rank = place + 1
            pid = np.random.default_rng(5).permutation(c.m).astype(U32)                         # (distinct ids: every entry written once)
            pos = _records(c, [c.phrase_start(int(k)) for k in order], "len")
            got = K.gk_phrase_ranks(K.GkCtx(c, tl, cl), pos, pid, K.sent(c.m + EXTRA, U32))
            want = GM.phrase_ranks(c, pos, pid, K.sent(c.m + EXTRA, U32))
            same(got, want, "%s %s %s" % (name, tl, cl))
            assert sorted(want[:c.m].tolist()) == list(range(1, c.m + 1))
            ran += 1
    assert ran == 4


def test_expand_entries():
    ran = 0
    for name in ("n=3x4096+1", "exception@4096"):
        for tl, cl in (("bytes", "bits"), ("packed", "list")):
            c = C.make_ctx(TEXTS[name], expand=1)
            D = int(c.pid.max()) + 1
            rng = np.random.default_rng(6)
            # legal: |alpha| = w (the suffix that begins w - 1 characters before its phrase end) and = phrase length - 1
            qs = [c.cuts[k] + 2 - c.w for k in range(0, len(c.cuts), 5)] + [c.phrase_start(k) + 1 for k in range(1, c.m, 7)] + _elements(c, 0, 8, 200)
            tab = np.zeros((D, 4), U32)
            tab[:, 0] = rng.integers(1, 9, D); tab[:, 1] = rng.integers(0, 1 << 20, D); tab[:, 2] = 1 << 20; tab[:, 3] = K.SENT32
            legal = []
            for q in qs:                                                                       # one phrase length per distinct id
                d = int(c.pid[c.phrase_of(q)])
                if int(tab[d, 2]) in (1 << 20, c.phrase_len(c.phrase_of(q))):
                    tab[d, 2] = c.phrase_len(c.phrase_of(q)); legal.append(q)
            pos = _records(c, legal, "len")
            forged = pos.copy()
            forged[1] = (int(pos[1]) & GM.POS_MASK) | ((c.w - 1) << 40)                         # |alpha| = w - 1: err[1]
            forged[2] = (int(pos[2]) & GM.POS_MASK) | (int(tab[int(c.pid[c.phrase_of(c.rec_pos(pos[2]))]), 2]) << 40)   # = the phrase length: err[1]
            for recs, n_err in ((pos, 0), (forged, 2)):
                B = len(recs)
                lcp = np.array([c.rec_len(r) - (1 if e % 3 == 0 else 0) + (5 if e % 3 == 2 else 0) for e, r in enumerate(recs)], dtype=U32)
                cols = lambda: dict({k: K.sent(B + EXTRA, U32) for k in ("cnt", "first", "offm1", "gs", "hl", "slen")}, bwt=K.sent(B + EXTRA, U8))
                err = lambda: np.concatenate([np.zeros(3, U32), K.sent(13, U32)])
                got = K.gk_expand_entries(K.GkCtx(c, tl, cl), recs, lcp, tab, cols(), err())
                want = GM.expand_entries(c, recs, lcp, tab, cols(), err())
                for k in want[0]:
                    same(got[0][k], want[0][k], "%s %s %s ce_%s" % (name, tl, cl, k))
                same(got[1], want[1], "err")
                assert int(want[1][1]) == n_err and want[0]["gs"][0] == 1 and 0 in want[0]["gs"][:B] and 1 in want[0]["gs"][1:B]
                ran += 1
    assert ran == 8


# ---- comparisons of phrase suffixes (without giant tables: see the header) -----------------------------------------------------
def _err():
    return np.concatenate([np.zeros(3, U32), K.sent(13, U32)])


def _small(loc, g, pos, ghead, slot, offset, limit, what, n_out):
    assert C.reject_compared(loc.c, pos, offset) is None
    mk = lambda: (K.sent(n_out, U64), K.sent(len(pos) + EXTRA, U8), _err(), K.sent(n_out, U32))
    got = K.gk_resolve_small(g, pos, ghead, slot, offset, *mk(), limit)
    want = GM.resolve_small(loc.c, pos, ghead, slot, offset, *mk(), limit)
    for g_, w_, name in zip(got, want, ("out", "flags", "err", "lcp_out")):
        same(g_, w_, what + " " + name)
    return want


def test_resolve_small():
    """pairs on the fast path (records with ranks) and on the general path (records with lengths), both text layouts, the
    phrase ends as bits and as a list (the fast path's `mask` is null then)"""
    offset, s = 21, 30
    ran = walked = same_alpha = 0
    for name, (muts, ends) in C.pair_cases(offset, s).items():
        for rec in ("rank", "len"):
            loc = C.Locus(muts, ends, rec=rec)
            pos = loc.members(s)
            q = [loc.c.rec_pos(r) for r in pos]
            order, shared = GM.alpha_cmp(loc.c, q[0], loc.c.rec_len(pos[0]), q[1], loc.c.rec_len(pos[1]))
            assert shared >= offset                                          # the group does share `offset` characters
            walked += rec == "rank" and order != 0 and shared >= offset + 32     # the pair path's walk behind its four words
            same_alpha += order == 0
            for tl, cl in (("bytes", "bits"), ("packed", "list")):
                for members in ((0, 1), (1, 0)):
                    want = _small(loc, K.GkCtx(loc.c, tl, cl), pos[list(members)], [0, 0], [5, 6], offset, 0,
                                  "%s %s %s %s %s" % (name, rec, tl, cl, members), 10)
                    assert int(want[2][1]) == (2 if name == "two_lengths" else 0)
                    assert (int(want[3][6]) != K.SENT32) == (order != 0)     # a hint where a character parts the two, none else
                    ran += 1
    assert ran == 13 * 2 * 2 * 2 and walked >= 4 and same_alpha >= 6


def test_resolve_small__ties_and_expansion():
    s, offset = 30, 21
    end = s + 149
    # equal ranks: the index decides
    loc = C.Locus([[], []], [end, end], rec="rank", ranks=np.zeros(7, U32))
    for members in ((0, 1), (1, 0)):
        want = _small(loc, K.GkCtx(loc.c, "packed", "bits"), loc.members(s)[list(members)], [0, 0], [0, 1], offset, 0, "equal ranks", 4)
        assert int(want[0][0]) == int(loc.members(s)[members[0]])
    # representatives: ties by position, the hint is |alpha|
    loc = C.Locus([[], [], [s + 90]], [end, end, end], rec="len", expand=1)
    pos = loc.members(s)
    for perm in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        want = _small(loc, K.GkCtx(loc.c, "bytes", "list"), pos[list(perm)], [0, 0, 0], [1, 2, 3], offset, 0, "expand %s" % (perm,), 6)
        hints = want[3][2:4].tolist()
        assert sorted(hints) == [90, 150]                                    # |alpha| between the two equal ones, 90 where the third parts


def test_resolve_small__group_sizes():
    """groups of 1, 2, 8 and 9 and one of three of which two spell the same alpha, with limit = 0 (eight) and = 3"""
    rng = np.random.default_rng(10)
    muts = [[], []] + [sorted(set(int(x) for x in rng.integers(60, 150, 2))) for _ in range(7)]
    ran = 0
    for rec in ("len", "rank"):
        loc = C.Locus(muts, [179] * 9, rec=rec)
        recs, ghead, slot = [], [], []
        for s, copies in ((30, [0]), (31, [3, 4]), (32, list(range(8))), (33, list(range(9))), (34, [2, 0, 1])):
            g0 = len(recs)
            recs += loc.members(s)[copies].tolist(); ghead += [g0] * len(copies); slot += [g0 + 3 + i for i in range(len(copies))]
        pos = np.array(recs, dtype=U64)
        for limit in (0, 3):
            for tl, cl in (("bytes", "bits"), ("packed", "list")):
                want = _small(loc, K.GkCtx(loc.c, tl, cl), pos, ghead, slot, 21, limit, "%s limit=%d %s" % (rec, limit, tl), len(pos) + 3 + EXTRA)
                flagged = sorted(set(int(ghead[e]) for e in range(len(pos)) if want[1][e]))
                assert [ghead.count(h) for h in flagged] == ([9] if limit == 0 else [8, 9])
                assert np.all(want[0][[slot[e] for e in range(len(pos)) if want[1][e]]] == U64(K.SENT64))     # left to the rounds
                ran += 1
    assert ran == 8


def _sorted_batch(loc, ss):
    c = loc.c
    recs = [int(r) for s in ss for r in loc.members(s)]
    v = bytes(c.vbyte(q) for q in range(c.n + 40))
    return np.array(sorted(recs, key=lambda r: (v[c.rec_pos(r):c.rec_pos(r) + c.rec_len(r)], c.rec_rank_key(r))), dtype=U64)


def test_batch_lcp():
    rng = np.random.default_rng(20)
    muts = [[], [], [], [], [95], [95], [120, 200], [260], [40]]
    ran = by_char = by_parse = 0
    for rec, expand in (("len", 0), ("rank", 0), ("len", 1)):
        loc = C.Locus(muts, [229] * 9, rec=rec, expand=expand)
        c = loc.c
        sl = rng.integers(0, 5000, c.m).astype(U32)
        pos = _sorted_batch(loc, (30, 31, 100))
        assert C.reject_compared(c, pos, 0) is None
        B = len(pos)
        for tl, cl in (("bytes", "bits"), ("packed", "list")):
            g = K.GkCtx(c, tl, cl)
            for carry, hints in ((None, False), (pos[:1].copy(), False), (None, True)):
                def mk():
                    l = np.concatenate([np.full(B, 0xFFFFFFFF, U32), K.sent(EXTRA, U32)])
                    if hints:
                        l[0] = 77; l[3] = 12345; l[B - 1] = 0                   # hints of the sort are kept (the first entry is not)
                    return l, _err()
                batch = pos[1:] if carry is not None else pos
                got = K.gk_batch_lcp(g, sl, batch, carry, *mk())
                want = GM.batch_lcp(c, sl, batch, carry, *mk())
                what = "%s expand=%d %s %s carry=%s hints=%s" % (rec, expand, tl, cl, carry is not None, hints)
                same(got[0][:len(batch) + EXTRA], want[0][:len(batch) + EXTRA], what + " lcp"); same(got[1], want[1], what + " err")
                assert int(want[1][2]) == 0
                ran += 1
            for j in range(1, B):
                o, _ = GM.alpha_cmp(c, c.rec_pos(pos[j]), c.rec_len(pos[j]), c.rec_pos(pos[j - 1]), c.rec_len(pos[j - 1]))
                by_char += o != 0; by_parse += o == 0
            # a pair in the wrong parse order (forged): err[2], and the value is the shorter alpha
            j = next(j for j in range(1, B) if GM.alpha_cmp(c, c.rec_pos(pos[j]), c.rec_len(pos[j]), c.rec_pos(pos[j - 1]), c.rec_len(pos[j - 1]))[0] == 0)
            bad = pos.copy(); bad[[j - 1, j]] = bad[[j, j - 1]]
            mk = lambda: (np.concatenate([np.full(B, 0xFFFFFFFF, U32), K.sent(EXTRA, U32)]), _err())
            got = K.gk_batch_lcp(g, sl, bad, None, *mk())
            want = GM.batch_lcp(c, sl, bad, None, *mk())
            same(got[0], want[0], "wrong order lcp"); same(got[1], want[1], "wrong order err")
            assert int(want[1][2]) == (0 if expand else 1) and int(want[0][j]) == c.rec_len(pos[j])
            ran += 1
    assert ran == 3 * 2 * 4 and by_char > 30 and by_parse > 30


def _medium_group(kinds, counts, rec, expand, seed, short=False, first_kind=0):
    """a locus whose copies are of the given kinds (lists of substitutions), counts[i] of kind i, shuffled; the member at the
    group's first place is of kind `first_kind`"""
    rng = np.random.default_rng(seed)
    order = [i for i, n_ in enumerate(counts) for _ in range(n_)]
    rng.shuffle(order)
    at = order.index(first_kind); order[0], order[at] = order[at], order[0]
    s, L = 30, 300
    ends = [s + L - 1] * len(order)
    if short:                                   # one member of the mutated kind ends its alpha inside the staged words
        ends[order.index(1)] = s + 21 + 5 + 20
    return C.Locus([kinds[i] for i in order], ends, seed=seed, rec=rec, expand=expand), order


def test_resolve_medium():
    """group sizes 9 .. 128 at the class boundaries, the copies of one locus in the layouts of guided_cases.medium_layouts;
    records with lengths (the reference member is chosen by pid), with pid absent, with ranks, representatives; both text
    layouts.  One group per launch here: a size class alone."""
    s, offset = 30, 21
    ran = second = third = 0
    modes = (("len", 0, True, "bytes", "bits"), ("len", 0, False, "packed", "list"), ("rank", 0, True, "packed", "bits"), ("len", 1, True, "bytes", "list"))
    for size in (9, 16, 17, 32, 33, 64, 65, 128):
        cl = GM.medium_class(size)
        for name, kinds in C.medium_layouts(32 if cl == 3 else 64).items():
            rec, expand, with_pid, tl, cl_ = modes[(ran + size) % 4]
            counts = [size - 2 * (len(kinds) - 1)] + [2] * (len(kinds) - 1) if len(kinds) > 1 else [size]
            if name in ("one_private", "short_alpha"):        # (the short alpha parts from every other member before it ends)
                counts = [size - 1, 1]
            for first_kind in ((0, 1) if name == "one_private" else (0,)):      # the private mutation is, and is not, the first member's
                loc, order = _medium_group(kinds, counts, rec, expand, size + ran, short=name == "short_alpha", first_kind=first_kind)
                c = loc.c
                if not with_pid:
                    c.pid = None
                pos = loc.members(s)
                assert C.reject_compared(c, pos, offset) is None
                sl = np.random.default_rng(ran).integers(0, 900, c.m).astype(U32)
                slot = np.arange(size, dtype=U32) + U32(4)
                classes = [[], [], [], []]; classes[cl] = [(0, size)]
                mk = lambda: (K.sent(size + 4 + EXTRA, U64), np.concatenate([np.ones(size, U8), K.sent(EXTRA, U8)]), _err(), K.sent(size + 4 + EXTRA, U32))
                got = K.gk_resolve_medium(K.GkCtx(c, tl, cl_), sl, pos, slot, classes, 3, offset, *mk())
                want = GM.resolve_medium(c, sl, pos, slot, classes, offset, *mk())
                what = "size=%d %s rec=%s expand=%d pid=%s %s first=%d" % (size, name, rec, expand, with_pid, tl, first_kind)
                for g_, w_, nm in zip(got, want, ("out", "flags", "err", "lcp_out")):
                    same(g_, w_, what + " " + nm)
                assert not want[1][:size].any() and int(want[2][1]) == 0
                lv = GM.medium_levels(c, pos, order.index(0))
                second += lv[0]; third += lv[1]
                ran += 1
    assert ran == 8 * 8 and second >= 40 and third >= 20


def test_resolve_medium__waves_and_forged_lengths():
    """several groups per class, so that a class's last wave holds one group and holds a full set (4 / 2 / 1 / 1 a wave); one
    group with two members that spell the same alpha with two lengths (forged phrase ends): err[1] grows by one for its wave"""
    s, offset = 30, 21
    ran = 0
    for n_small in (5, 8):                                              # class 0: the last wave holds 1 group, and 4
        for forged in (False, True):
            sizes = [9 + (i % 8) for i in range(n_small)] + [20, 30, 17] + [40] + [70]
            muts = [[], [s + 40], [s + 40], [s + 90]] * 32
            ends = [s + 299] * 128
            if forged:
                ends[1] = s + 200; ends[2] = s + 180                        # copies 1 and 2: one alpha, two lengths
            loc = C.Locus(muts[:70], ends[:70], seed=n_small, rec="len")
            c = loc.c
            recs, classes, slot = [], [[], [], [], []], []
            for size in sizes:
                g0 = len(recs)
                recs += loc.members(s + len(classes[0]) % 3)[:size].tolist()
                classes[GM.medium_class(size)].append((g0, size))
                slot += [g0 + 2 + i for i in range(size)]
            pos = np.array(recs, dtype=U64)
            m = len(pos)
            sl = np.random.default_rng(1).integers(0, 900, c.m).astype(U32)
            mk = lambda: (K.sent(m + 2 + EXTRA, U64), np.concatenate([np.ones(m, U8), K.sent(EXTRA, U8)]), _err(), K.sent(m + 2 + EXTRA, U32))
            got = K.gk_resolve_medium(K.GkCtx(c, "packed", "bits"), sl, pos, slot, classes, 8, offset, *mk())
            want = GM.resolve_medium(c, sl, pos, slot, classes, offset, *mk())
            for g_, w_, nm in zip(got, want, ("out", "flags", "err", "lcp_out")):
                same(g_, w_, "n_small=%d forged=%s %s" % (n_small, forged, nm))
            waves = (n_small + 3) // 4 + 2 + 1 + 1
            assert int(want[2][1]) == (waves if forged else 0)              # every group holds copies 1 and 2
            ran += 1
    assert ran == 4


# ---- cases the wrappers' own tests above leave out ---------------------------------------------------------------------------------
def test_batch_fill__no_code_for_a_base():
    """a packed text of A, C and T with its own code table: G has no code, so no tile may be read as 2-bit words (dense_ok = 0)
    although every other condition holds -- histogram, counts, fill and staging against the model"""
    text = C.three_base_text()
    own = GM.code_table(text)
    c, c_full = C.make_ctx(text, code=own), C.make_ctx(text)
    assert int(own[0][ord("G")]) == 0 and GM.dense_tiles(c, "packed") == [] and GM.dense_tiles(c_full, "packed") == [0, 1, 2]
    g = K.GkCtx(c, "packed", "list")
    pc = 3
    nb = 1 << (c.bits * pc)
    mk = lambda: np.concatenate([np.zeros(nb, U64), K.sent(EXTRA, U64)])
    same(K.gk_bin_hist(g, pc, mk()), GM.bin_hist(c, pc, mk()), "bin_hist")
    ran = 0
    for lo, hi in ((0, nb), (nb // 3, nb // 2), (5, 5)):
        counts = GM.batch_count(c, pc, lo, hi, K.sent(c.tiles + EXTRA, U32))
        same(K.gk_batch_count(g, pc, lo, hi, K.sent(c.tiles + EXTRA, U32)), counts, "batch_count [%d, %d)" % (lo, hi))
        off, total = _tile_offsets_of(counts[:c.tiles], gap=1)
        mk2 = lambda: (K.sent(total + 4096 + EXTRA, U64), K.sent(total + 4096 + EXTRA, U64), K.sent(c.tiles + EXTRA, U32))
        got = K.gk_batch_fill(g, pc, lo, hi, off, *mk2()[:2], 0, nb, mk2()[2])
        want = GM.batch_fill(c, pc, lo, hi, off, *mk2()[:2], 0, nb, mk2()[2])
        for g_, w_, nm in zip(got, want, ("keys", "records", "next_count")):
            same(g_, w_, "batch_fill [%d, %d) %s" % (lo, hi, nm))
        gs = K.gk_stage_fill(g, pc, lo, hi, off, K.sent(total + 4096 + EXTRA, U32), 0, 0, None)
        ws = GM.stage_fill(c, pc, lo, hi, off, K.sent(total + 4096 + EXTRA, U32), 0, 0, None)
        same(gs[0], ws[0], "stage_fill [%d, %d)" % (lo, hi))
        ran += 1
    assert ran == 3


def test_batch_fill__every_position_of_the_cut_cases_in_both_layouts():
    """every text position of every mask of guided_cases.cut_cases queried on the device, through batch_fill over all bins:
    records with lengths ask next_cut (alpha_len; with the expansion's filter on, a plain tile takes the end from the staged
    phrase ends instead), records with ranks ask rank1 (isa_p[k] = k: the record spells the rank).  The bit layout and the
    list layout (list_lower: blocks of 0, 1, 8, 9, 64, 65 and 513 phrase ends) give the same output, the model's."""
    ran = queried = 0
    for name, (n, cuts) in C.cut_cases().items():
        text = C._bases(np.random.default_rng(n), n)
        m = len(cuts) + 1
        code, bits, chars = C.full_code()
        for tl, rec, rep in (("bytes", "len", None), ("packed", "len", "all"), ("bytes", "rank", None), ("packed", "rank", "all")):
            c = GM.Ctx(text, 5, cuts, code, bits, chars, pos_bits=20 if rec == "rank" else 40, rec_rank=1 if rec == "rank" else 0,
                       isa_p=np.arange(m, dtype=U32), rep=None if rep is None else [1] * m)
            off, total = _tile_offsets_of([min(4096, n - 4096 * t) for t in range(c.tiles)])
            assert total == n
            mk = lambda: (K.sent(n + 4096 + EXTRA, U64), K.sent(n + 4096 + EXTRA, U64))
            want = GM.batch_fill(c, 1, 0, 1 << bits, off, *mk(), 0, 0, None)
            out = {}
            for cl in ("bits", "list"):
                out[cl] = K.gk_batch_fill(K.GkCtx(c, tl, cl), 1, 0, 1 << bits, off, *mk(), 0, 0, None)
                same(out[cl][0], want[0], "%s %s %s %s keys" % (name, tl, rec, cl))
                same(out[cl][1], want[1], "%s %s %s %s records" % (name, tl, rec, cl))
                queried += n
            same(out["bits"][1], out["list"][1], "%s: the two layouts" % name)
            if rec == "rank":           # the ranks the records spell, against a plain count
                assert [int(r) >> 20 for r in want[1][:n:97]] == [(sum(1 for x in cuts if x < min(p + 4, n)) + 1) % m if sum(1 for x in cuts if x < min(p + 4, n)) + 1 < m else 0 for p in range(0, n, 97)]
            ran += 1
    assert ran == 13 * 4 and queried > 600000


def test_resolve_medium__phrases_exceptions_and_full_waves():
    s, offset = 30, 21
    # (1) a list of phrases (skip = 1) with forged duplicates: equal phrases keep their order, err[0] counts the wave
    muts = [[], [], [80], [], [], [80, 200], [], [], [], []]
    loc = C.Locus(muts, [s + 299] * 10, rec="len", skip=1)
    c = loc.c
    pos = loc.phrases()
    assert C.reject_compared(c, pos, offset) is None and len(set(int(r) >> 40 for r in pos)) == 1
    sl = np.zeros(c.m, U32)
    slot = np.arange(10, dtype=U32) + U32(2)
    for tl, cl in (("bytes", "bits"), ("packed", "list")):
        mk = lambda: (K.sent(12 + EXTRA, U64), np.concatenate([np.ones(10, U8), K.sent(EXTRA, U8)]), _err(), K.sent(12 + EXTRA, U32))
        got = K.gk_resolve_medium(K.GkCtx(c, tl, cl), sl, pos, slot, [[(0, 10)], [], [], []], 2, offset, *mk())
        want = GM.resolve_medium(c, sl, pos, slot, [[(0, 10)], [], [], []], offset, *mk())
        for g_, w_, nm in zip(got, want, ("out", "flags", "err", "lcp_out")):
            same(g_, w_, "phrases %s %s" % (tl, nm))
        assert int(want[2][0]) == 1 and int(want[2][1]) == 0
        assert [int(x) for x in want[0][2:10]] == [int(pos[i]) for i in (0, 1, 3, 4, 6, 7, 8, 9)]      # the eight equal ones, by index
    # (2) a packed text, one member with an N inside the 64 characters the kernel stages: its codes cannot be read as words
    ran = 0
    for n_pos in (s + offset + 3, s + offset + 63, s + offset + 70):
        muts = [[]] * 6 + [[s + offset + 40]] * 2 + [[]] * 4
        loc = C.Locus(muts, [s + 299] * 12, rec="len", n_at={3: [n_pos], 7: [n_pos]})
        c = loc.c
        pos = loc.members(s)
        sl = np.random.default_rng(2).integers(0, 90, c.m).astype(U32)
        slot = np.arange(12, dtype=U32)
        mk = lambda: (K.sent(12 + EXTRA, U64), np.concatenate([np.ones(12, U8), K.sent(EXTRA, U8)]), _err(), K.sent(12 + EXTRA, U32))
        readable = [GM.codes64_readable(c, c.rec_pos(r) + offset) for r in pos]
        assert not readable[3] and not readable[7] and any(readable), readable       # both ways of staging in one group
        got = K.gk_resolve_medium(K.GkCtx(c, "packed", "bits"), sl, pos, slot, [[(0, 12)], [], [], []], 1, offset, *mk())
        want = GM.resolve_medium(c, sl, pos, slot, [[(0, 12)], [], [], []], offset, *mk())
        for g_, w_, nm in zip(got, want, ("out", "flags", "err", "lcp_out")):
            same(g_, w_, "N at %d %s" % (n_pos, nm))
        ran += 1
    # (3) two and four groups of the class of 17 .. 32 (two a wave: the last wave full), one and two of the larger classes
    loc = C.Locus([[], [s + 40], [s + 40], [s + 90]] * 20, [s + 299] * 80, seed=3, rec="rank")
    c = loc.c
    for n1 in (2, 4):
        sizes = [20, 32, 17, 25][:n1] + [40, 64] + [70]
        recs, classes, slot = [], [[], [], [], []], []
        for i, size in enumerate(sizes):
            g0 = len(recs)
            recs += loc.members(s + i % 3)[:size].tolist()
            classes[GM.medium_class(size)].append((g0, size)); slot += [g0 + i for i in range(size)]
        pos = np.array(recs, dtype=U64); m = len(pos)
        sl = np.random.default_rng(1).integers(0, 900, c.m).astype(U32)
        mk = lambda: (K.sent(m + EXTRA, U64), np.concatenate([np.ones(m, U8), K.sent(EXTRA, U8)]), _err(), K.sent(m + EXTRA, U32))
        got = K.gk_resolve_medium(K.GkCtx(c, "bytes", "list"), sl, pos, slot, classes, 4, offset, *mk())
        want = GM.resolve_medium(c, sl, pos, slot, classes, offset, *mk())
        for g_, w_, nm in zip(got, want, ("out", "flags", "err", "lcp_out")):
            same(g_, w_, "n1=%d %s" % (n1, nm))
        assert len(classes[1]) == n1 and len(classes[2]) == 2
        ran += 1
    assert ran == 5


def _in_giant(c, rec):
    return c.giant_entry(c.rec_pos(rec), 0) is not None


def test_batch_lcp__pairs_decided_by_the_giant_dictionary():
    """a real dictionary of the phrases longer than g_depth = 42: neighbours whose alphas run on for more than 64 characters
    and first differ behind them are ordered, and their LCP is read (stop + the range minimum of the dictionary's LCP array),
    without a walk through the text -- the value must be the true LCP; also resolve_small and resolve_medium on such members,
    with equal and with different groups of the dictionary"""
    s, offset = 30, 21
    muts = [[], [], [], [s + 100], [s + 100], [s + 100, s + 230], [s + 180], [s + 95], [s + 64], [s + 65], [s + 66], [s + 250]]
    ran = by_dict = 0
    for rec in ("len", "rank"):
        loc = C.Locus(muts, [s + 299] * 12, rec=rec, g_depth=42)
        c = loc.c
        assert sum(c.giant.flag) >= 12 and len(set(c.giant.grp.tolist())) < len(c.giant.grp)
        sl = np.random.default_rng(4).integers(0, 900, c.m).astype(U32)
        pos = _sorted_batch(loc, (s, s + 1))
        B = len(pos)
        assert C.reject_compared(c, pos, 0) is None and all(_in_giant(c, r) for r in pos)
        for j in range(1, B):
            o, t = GM.alpha_cmp(c, c.rec_pos(pos[j]), c.rec_len(pos[j]), c.rec_pos(pos[j - 1]), c.rec_len(pos[j - 1]))
            by_dict += o != 0 and t >= 64
        for tl, cl in (("bytes", "bits"), ("packed", "list")):
            g = K.GkCtx(c, tl, cl)
            mk = lambda: (np.concatenate([np.full(B, 0xFFFFFFFF, U32), K.sent(EXTRA, U32)]), _err())
            got = K.gk_batch_lcp(g, sl, pos, None, *mk())
            want = GM.batch_lcp(c, sl, pos, None, *mk())
            same(got[0], want[0], "%s %s lcp" % (rec, tl)); same(got[1], want[1], "%s %s err" % (rec, tl))
            # the same members as one small group each of two, and as one medium group of twelve
            members = loc.members(s)
            for a, b in ((3, 5), (5, 3), (0, 11), (8, 9), (9, 10), (0, 1)):
                _small(loc, g, members[[a, b]], [0, 0], [3, 4], offset, 0, "%s %s pair (%d, %d)" % (rec, tl, a, b), 8)
            slot = np.arange(12, dtype=U32)
            mk3 = lambda: (K.sent(12 + EXTRA, U64), np.concatenate([np.ones(12, U8), K.sent(EXTRA, U8)]), _err(), K.sent(12 + EXTRA, U32))
            gotm = K.gk_resolve_medium(g, sl, members, slot, [[(0, 12)], [], [], []], 1, offset, *mk3())
            wantm = GM.resolve_medium(c, sl, members, slot, [[(0, 12)], [], [], []], offset, *mk3())
            for g_, w_, nm in zip(gotm, wantm, ("out", "flags", "err", "lcp_out")):
                same(g_, w_, "%s %s medium %s" % (rec, tl, nm))
            ran += 1
    assert ran == 4 and by_dict >= 8


def test_batch_count__forged_leads_above_the_symbol():
    """a run of N at the end of a text that ends with a tile, continued by a forged table entry and followed by T (above N) and
    by A (below): r = 2^8 .. 2^40 + 5 reach run_bucket in the class of followers above the symbol too"""
    text = C._bases(np.random.default_rng(3), 2 * 4096, b"ACG")
    text[-10:] = ord("N")
    c = C.make_ctx(text)
    sym, pc = int(c.code[ord("N")]), 2
    bin_ = (sym << c.bits) | sym
    ran = 0
    seen = set()
    for R in FORGED_R:
        for follow in (int(c.code[ord("T")]), int(c.code[ord("A")])):
            first, whole, fol = _run_tables(c, sym, (R - 5, follow))
            for blo, bhi in ((0, 2 * HALF), (0, HALF), (HALF, 2 * HALF)):
                rs = GM.RunSlice(sym, blo, bhi, whole, first, fol)
                seen |= {GM.run_at(c, rs, p) for p in range(c.n - 10, c.n)}
                for tl in LAYOUTS:
                    same(K.gk_batch_count(K.GkCtx(c, tl), pc, bin_, bin_ + 1, K.sent(c.tiles + EXTRA, U32), rs),
                         GM.batch_count(c, pc, bin_, bin_ + 1, K.sent(c.tiles + EXTRA, U32), rs), "R=%d follow=%d [%d, %d)" % (R, follow, blo, bhi))
                    ran += 1
            mk = lambda: np.concatenate([np.zeros(4 * HALF, U64), K.sent(EXTRA, U64)])
            same(K.gk_run_hist(K.GkCtx(c, "bytes"), pc, bin_, rs, mk()), GM.run_hist(c, pc, bin_, rs, mk()), "R=%d run_hist" % R)
    assert ran == 5 * 2 * 3 * 2
    assert any(b >= HALF for _, b in seen) and any(0 < b < HALF for _, b in seen) and (2 ** 40 + 5, HALF) in seen and (2 ** 32 + 1, GM.run_bucket(2 ** 32 + 1, False)) in seen
