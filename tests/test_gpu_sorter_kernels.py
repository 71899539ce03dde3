"""The suffix sorter's kernels and range sorts, one launch wrapper at a time, against plain references (tests/kprobe.py)
through the probe library (tests/kprobe/kprobe.cpp).  Every comparison is exact; every input satisfies the
preconditions kernels.hpp / prims.hpp document.  Routes chosen by a switch that is read once per process run in a child
process (tests/sorter_cases.py), one child per setting."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kprobe as K
import sorter_cases as C
from kprobe import U8, U32, U64, SENT32, NO_SEP

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_child(groups, env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "sorter_cases.py")] + list(groups), env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sorter cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


# ---- first keys -----------------------------------------------------------------------------------------------------
def _ident_code(bits):
    code = np.zeros(256, U8)
    code[:1 << bits] = np.arange(1 << bits)
    return code


@pytest.mark.parametrize("bits,chars,sep", [(2, 32, NO_SEP), (3, 21, NO_SEP), (4, 16, NO_SEP), (2, 31, 1), (3, 21, 5), (4, 15, 0),
                                            (7, 9, 3)])
def test_pack_keys(bits, chars, sep):
    rng = np.random.default_rng(bits * 100 + chars)
    code = _ident_code(bits)
    for n in (1, chars - 1, chars, 1023, 1024, 1025):
        text = rng.integers(1, 1 << bits, n).astype(U8)
        if sep != NO_SEP:
            text[rng.random(n) < 0.08] = sep
            text[-1] = sep                                 # a text with terminators ends in one
        keys, vals = K.pack_keys(text, code, bits, chars, sep)
        assert np.array_equal(vals, np.arange(n, dtype=U32))
        want = K.ref_pack_keys(code[text], bits, chars, sep)
        assert np.array_equal(keys, want), (n, np.flatnonzero(keys != want)[:5])


@pytest.mark.parametrize("bits,chars", [(2, 31), (3, 21)])
def test_pack_keys_run_ends(bits, chars):
    a, b = 2, 3
    text = [a] * (chars + 1) + [b] + [a] * (chars - 1) + [b] + [a] * chars + [b] + [a] * chars + [1] + [b] * (2 * chars) + [a] * chars
    pad = 1500 - len(text)
    text = u = text[:3 * chars + 3] + [b, a] * (pad // 2) + text[3 * chars + 3:]      # runs in several workgroups' tiles
    text = np.array(u, U8)
    code = _ident_code(bits)
    want = K.ref_run_ends(code[text].tolist(), chars)
    assert len(want) == 5 and want[0] == chars and want[-1] == len(text) - 1
    keys, vals, ends, cnt = K.pack_keys(text, code, bits, chars, 1, run_alloc=16, run_cap=16)
    assert cnt == len(want) and sorted(ends[:cnt].tolist()) == want and np.all(ends[cnt:] == SENT32)
    assert np.array_equal(keys, K.ref_pack_keys(code[text], bits, chars, 1))
    keys, vals, ends, cnt = K.pack_keys(text, code, bits, chars, 1, run_alloc=16, run_cap=3)
    assert cnt == len(want), "every run is counted, listed or not"
    assert set(ends[:3].tolist()) <= set(want) and len(set(ends[:3].tolist())) == 3 and np.all(ends[3:] == SENT32)


@pytest.mark.parametrize("bits,chars", [(21, 3), (16, 4), (1, 64), (13, 4)])
def test_pack_keys_u32(bits, chars):
    rng = np.random.default_rng(bits)
    for m in (1, chars - 1, chars, 1023, 1024, 1025):
        if m < 1:
            continue
        parse = rng.integers(1, 1 << bits, m).astype(U32)
        keys, vals = K.pack_keys_u32(parse, bits, chars)
        assert np.array_equal(vals, np.arange(m, dtype=U32))
        assert np.array_equal(keys, K.ref_pack_keys_u32(parse, bits, chars))


# ---- heads and ranks ------------------------------------------------------------------------------------------------
def _bucket_lists(n):
    """bucket sizes that add up to n: all singletons, one bucket, random with a tie that includes the last element"""
    out = [[1] * n, [n]]
    if n > 2:
        rng = np.random.default_rng(n)
        sizes = []
        while sum(sizes) < n - 2:
            sizes.append(int(min(rng.integers(1, 6), n - 2 - sum(sizes))))
        out.append(sizes + [2])
    return out


def _head_column(sizes):
    return U32(np.repeat(np.cumsum([0] + sizes[:-1]), sizes))


SIZES = (1, 2, 255, 256, 257)


@pytest.mark.parametrize("n", SIZES)
def test_mark_heads_force_heads(n):
    for sizes in _bucket_lists(n):
        keys = (np.repeat(np.arange(len(sizes)), sizes).astype(U64) * U64(6)) | (U64(1) << U64(63))
        for lsb in (0, 1):
            k = keys.copy()
            if lsb:
                k[np.arange(n) % 3 == 0] |= U64(1)            # unique terminators: buckets of their own
                k = np.sort(k)
            headval = np.empty(n, U32)
            K.call("mark_heads", k, n, lsb, headval)
            assert np.array_equal(headval, K.ref_mark_heads(k, lsb))
        at = U32([0, n - 1, n, n // 2])                      # (a position at n is ignored: the end of the last bucket)
        K.call("force_heads", headval, n, at, len(at))
        want = K.ref_mark_heads(k, 1)
        want[[0, n - 1, n // 2]] = [0, n - 1, n // 2]
        assert np.array_equal(headval, want)


@pytest.mark.parametrize("n", SIZES)
def test_scatter_rank_and_changed(n):
    rng = np.random.default_rng(n)
    for sizes in _bucket_lists(n):
        head = _head_column(sizes)
        sa = U32(rng.permutation(n + 3))[:n].copy()            # (the rank column is longer than the list)
        rank = np.full(n + 3, SENT32, U32)
        K.call("scatter_rank", sa, head, n, rank, n + 3)
        want = np.full(n + 3, SENT32, U32); want[sa] = head
        assert np.array_equal(rank, want)
        old = head.copy()
        changed = rng.random(n) < 0.3
        changed[-1] = n % 2 == 1
        old[changed] += U32(1000)
        rank = np.full(n + 3, SENT32, U32)
        K.call("scatter_rank_changed", sa, head, old, n, rank, n + 3)
        want = np.full(n + 3, SENT32, U32); want[sa[changed]] = head[changed]
        assert np.array_equal(rank, want), "a rank whose head did not change was written (or one that changed was not)"


@pytest.mark.parametrize("n", SIZES + (4095, 4096, 4097, 4113))
def test_select_tied_heads_is_flag_then_select(n):
    for sizes in _bucket_lists(n):
        head = _head_column(sizes)
        flags = np.empty(n, U8)
        K.call("flag_unsorted", head, n, flags)
        assert np.array_equal(flags, K.ref_flag_unsorted(head))
        want = U32(np.flatnonzero(flags))
        for which in ("select_indices", "select_tied_heads"):
            out = np.full(n, SENT32, U32); cnt = np.full(1, SENT32, U32)
            K.call(which, flags if which == "select_indices" else head, n, out, cnt)
            assert int(cnt[0]) == len(want), which
            assert np.array_equal(out[:len(want)], want) and np.all(out[len(want):] == SENT32), which
    assert len(_bucket_lists(n)[0]) == n                      # (the lists above hold a count of 0 and a count of n)


@pytest.mark.parametrize("m", SIZES)
def test_gather_compact_subheads(m):
    rng = np.random.default_rng(m)
    n = 3 * m + 5
    sa = U32(rng.permutation(n)); head = U32(np.sort(rng.integers(0, n, n)))
    idx = U32(np.sort(rng.choice(n, m, replace=False)))
    op, os_, oh = (np.empty(m, U32) for _ in range(3))
    K.call("gather_active", idx, m, sa, head, n, op, os_, oh)
    assert np.array_equal(op, idx) and np.array_equal(os_, sa[idx]) and np.array_equal(oh, head[idx])
    K.call("compact_round", idx, m, U32(np.arange(n) * 2), sa, head, n, op, os_, oh)
    assert np.array_equal(op, idx * 2) and np.array_equal(os_, sa[idx]) and np.array_equal(oh, head[idx])
    for sizes in _bucket_lists(m):
        keys = np.repeat(np.arange(len(sizes)), sizes).astype(U64) << U64(61)
        pos = U32(np.sort(rng.choice(n, m, replace=False)))
        hv = np.empty(m, U32)
        K.call("mark_subheads", keys, pos, m, hv)
        assert np.array_equal(hv, K.ref_mark_subheads(keys, pos))


@pytest.mark.parametrize("m", SIZES)
def test_apply_round(m):
    """SA[pos[c]] = sa_sorted[c]; rank[sa_sorted[c]] = newhead[c]; flags[c] = still unsorted -- nothing else is written"""
    rng = np.random.default_rng(m)
    n = 2 * m + 7
    for sizes in _bucket_lists(m):
        pos = U32(np.sort(rng.choice(n, m, replace=False)))
        newhead = pos[_head_column(sizes)]                     # the position of the first element of every new bucket
        sa_sorted = U32(rng.permutation(n)[:m])
        sa = np.full(n, SENT32, U32); rank = np.full(n, SENT32, U32); flags = np.full(m, K.SENT8, U8)
        K.call("apply_round", sa_sorted, newhead, pos, m, sa, rank, n, flags)
        want_sa = np.full(n, SENT32, U32); want_sa[pos] = sa_sorted
        want_rank = np.full(n, SENT32, U32); want_rank[sa_sorted] = newhead
        assert np.array_equal(sa, want_sa) and np.array_equal(rank, want_rank)
        want_flags = np.repeat(np.array(sizes) > 1, sizes).astype(U8)      # a bucket of one is sorted, the last element included
        assert np.array_equal(flags, want_flags) and np.array_equal(flags, K.ref_round_flags(newhead, pos))


# ---- round keys -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 3, 4, 5, 1027))
def test_round_keys_both_kernels(m):
    rng = np.random.default_rng(m)
    n = 2 * m + 40
    rank = U32(rng.integers(0, n, n))
    sac = U32(rng.permutation(n)[:m])
    sac[0] = 5
    sac[-1] = n - 1
    target = 512
    n_tiles = (m + target - 1) // target
    marks = np.zeros(n_tiles + 1, U8)
    marks[:n_tiles] = 1
    marks[0] |= 2; marks[n_tiles - 1] |= 4                    # one long range over the whole list
    bound = np.full(n_tiles + 1, K.NO_BOUND, U32); bound[0] = 0; bound[n_tiles] = m
    low_heads = U32(np.sort(rng.integers(0, n, m)))
    high_heads = U32(np.sort(rng.integers(0x3FFFFFF0, 0xFFFFFFF0, m, dtype=np.int64)))
    high_heads[0] = 0x40000000
    high_heads[-1] = 0xFFFFFFF0
    for headc, shift in ((low_heads, K.bit_width(n)), (high_heads, 32)):
        # h: inside the text, past its end for some, the largest step, and 2^32 - sa[0] (a 32-bit sum wraps into the text)
        for h in (1, n // 2, n, 0xFFFFFFFF, (1 << 32) - 5):
            want = K.ref_round_keys(sac, headc, rank, n, h, shift)
            keys = np.empty(m, U64)
            K.call("make_round_keys", sac, headc, m, rank, n, n, K.c_u32(h), shift, keys)
            assert np.array_equal(keys, want), ("make_round_keys", h, shift)
            big = np.full(m, K.SENT64, U64)
            K.call("round_big_keys", marks, bound, target, n_tiles, sac, headc, m, rank, n, n, K.c_u32(h), shift, big)
            assert np.array_equal(big, want), ("round_big_keys", h, shift)
            if h >= n:
                assert np.all(want & U64((1 << shift) - 1) == 0)          # past the end: the second component is 0
        if shift == 32:
            assert int(want[-1]) >> 63 == 1 and any((int(x) >> 62) & 1 for x in want)


# ---- one round, in its two forms --------------------------------------------------------------------------------------
def test_round_forms_default_tile():
    """round_head_bounds + round_fused + k_big_* and round_tile_bounds + round_local_sort, tiles of 2048"""
    assert K.lib().kp_round_fused_cap() == 2048
    assert C.round_cases() > 0


def test_round_forms_small_tile():
    """the same with tiles of 1024 (MMT_ROUND_CAP, read once: a child process)"""
    run_child(["round"], {"MMT_ROUND_CAP": "1024"})


# ---- run refinement ---------------------------------------------------------------------------------------------------
def test_equal_range_u64():
    sorted_keys = np.repeat(np.array([3, 9, 9, 1 << 63, (1 << 64) - 2], dtype=U64), [4, 1, 6, 5, 2])
    probe = np.array([3, (1 << 64) - 2, 4, 0, (1 << 64) - 1, 1 << 63, 9], dtype=U64)
    out = np.empty(2 * len(probe), U32)
    K.call("equal_range_u64", sorted_keys, len(sorted_keys), probe, len(probe), out)
    assert np.array_equal(out, K.ref_equal_range(sorted_keys, probe))
    same = np.full(300, 7, U64)
    K.call("equal_range_u64", same, 300, np.array([7], dtype=U64), 1, out)
    assert out[:2].tolist() == [0, 300]


def test_run_keys_order_the_bucket():
    """key2[a] < key2[b] implies suffix a < suffix b, for the suffixes that begin with `chars` copies of one symbol"""
    rng = np.random.default_rng(3)
    bits, chars = 3, 21
    code = np.zeros(256, U8); code[2:8] = np.arange(1, 7)      # bytes 0 and 1 are terminators (code 0)
    c = 4                                                      # the run symbol: symbols below and above it follow runs
    parts = []
    for i in range(60):
        parts += [c] * int(rng.integers(chars - 2, chars + 40))
        parts += [[2], [7], [1], [3, c, 5], [6, 6, 1], [2, c]][i % 6]
    text = np.array(parts + [0], U8)
    sym = code[text]
    n = len(text)
    ends = U32(K.ref_run_ends(sym.tolist(), chars))
    bucket = U32([p for p in range(n - chars + 1) if np.all(sym[p:p + chars] == code[c])])
    assert len(bucket) > 300
    key2 = np.empty(len(bucket), U64)
    K.call("run_keys", bucket, len(bucket), text, n, code, bits, chars, ends, len(ends), key2)
    true_rank = np.empty(n, np.int64)
    true_rank[K.ref_suffix_array(sym, terminator=0)] = np.arange(n)
    order = np.lexsort((true_rank[bucket], key2))
    k_sorted, r_sorted = key2[order], true_rank[bucket][order]
    assert np.all(r_sorted[1:] > r_sorted[:-1]), "a smaller key on a larger suffix"
    assert len(np.unique(k_sorted)) > 50


# ---- prims: range sorts -----------------------------------------------------------------------------------------------
def test_range_sorts_default_routes():
    """short ranges share the segmented sort (no range is giant); keys that order the ranges go through one sort"""
    assert C.range_cases(300) > 0


def test_range_sorts_tagged_and_giant_routes():
    """MMT_GIANT_RANGE=64: 32-bit keys take the one sort of tagged keys; 64-bit keys split into device-wide sorts of
    the giant ranges and a segmented sort of the others (a single range: all giant)"""
    run_child(["ranges_small"], {"MMT_GIANT_RANGE": "64"})


def test_range_sorts_older_routes():
    """MMT_RANGES_AS_ONE=0: all four type pairs through the giant / segmented split"""
    run_child(["ranges_small"], {"MMT_GIANT_RANGE": "64", "MMT_RANGES_AS_ONE": "0"})


def test_tagged_route_in_process():
    """a range beyond half the default giant threshold: the tagged sort without any switch, end_bit below 32 with garbage above"""
    # Which route runs is not observable from outside: it follows from prims.hip (sort_ranges), GIANT = 65536 by default and
    # "any range longer than GIANT / 2" for 32-bit keys.  Should those thresholds move, this test still checks a correct
    # sort but of another route; the children with MMT_GIANT_RANGE=64 (test_range_sorts_tagged_and_giant_routes) pin the
    # tagged route independently of the default.  The same holds for the route names in the docstrings of the range tests.
    rng = np.random.default_rng(5)
    n = 33200
    kin = U32(rng.integers(0, 1 << 11, n)) | (U32(rng.integers(1, 1 << 20, n)) << U32(11))
    vin = U64(rng.integers(0, 1 << 62, n))
    begin, end = [33000, 100], [33150, 100 + 32769]
    kout, vout = K.sort_ranges(kin, vin, begin, end, 11)
    C._check_ranges(kin, vin, kout, vout, begin, end, 11)


def test_sort_pairs_u64_u32_is_stable():
    rng = np.random.default_rng(9)
    for n in (1, 2, 257, 5000):
        kin = (U64(rng.integers(0, 7, n)) << U64(61)) | U64(rng.integers(0, 3, n))
        vin = U32(rng.permutation(n))
        kout = np.empty(n, U64); vout = np.empty(n, U32)
        K.call("sort_pairs_u64_u32", kin, vin, n, 0, 64, kout, vout)
        order = np.argsort(kin, kind="stable")
        assert np.array_equal(kout, kin[order]) and np.array_equal(vout, vin[order]), "refine_runs relies on a stable sort"


# ---- prims: scans -----------------------------------------------------------------------------------------------------
SCAN_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 5000)


def test_inclusive_max_in_place():
    rng = np.random.default_rng(1)
    for n in SCAN_SIZES + ((1 << 22) - 1, (1 << 22) + 4099):      # the library scan below 2^22 elements, the two-pass one above
        a = U32(rng.integers(0, 1 << 32, n, dtype=np.int64))
        a[rng.random(n) < 0.7] = 0
        assert np.array_equal(K.scan(0, a, U32), np.maximum.accumulate(a)), n


def _ref_segmin(a):
    out = np.empty(len(a), U64)
    cur = None
    for i, x in enumerate(a.tolist()):
        if cur is None or x >> 32:
            cur = x
        else:
            cur = (cur & 0xFFFFFFFF00000000) | min(cur & 0xFFFFFFFF, x & 0xFFFFFFFF)
        out[i] = cur
    return out


def test_inclusive_segmin_in_place():
    rng = np.random.default_rng(2)
    for n in SCAN_SIZES:
        val = U64(rng.integers(0, 1 << 32, n, dtype=np.int64))
        for heads in ([0], [0, n - 1], [0, 1, 2, n // 2, n // 2 + 1], sorted(set([0] + rng.integers(0, n, n // 9).tolist()))):
            flag = np.zeros(n, U64)
            flag[[h for h in heads if h < n]] = 1              # [0] alone: one segment over several workgroups
            a = (flag << U64(32)) | val
            assert np.array_equal(K.scan(1, a, U64), _ref_segmin(a)), (n, heads[:5])


def test_sums():
    rng = np.random.default_rng(3)
    for n in SCAN_SIZES:
        a = U32(rng.integers(0, 1 << 20, n))
        inc = np.cumsum(a.astype(np.uint64))
        assert np.array_equal(K.scan(3, a, U32), inc.astype(U32))
        assert np.array_equal(K.scan(2, a, U32), (inc - a).astype(U32))
        big = U32(rng.integers(0xC0000000, 1 << 32, n, dtype=np.int64))
        inc = np.cumsum(big.astype(np.uint64))
        assert np.array_equal(K.scan(4, big, U64), inc - big), "a 32-bit accumulator"
        big64 = U64(rng.integers(0, 1 << 62, n, dtype=np.int64))
        inc = np.cumsum(big64)
        assert np.array_equal(K.scan(5, big64, U64), inc - big64)
    three = U32([0xC0000000] * 3)
    assert K.scan(4, three, U64).tolist() == [0, 0xC0000000, 0x180000000]
    assert K.scan(5, three.astype(U64), U64).tolist() == [0, 0xC0000000, 0x180000000]


def test_probe_reports_errors():
    with pytest.raises(K.ProbeError, match="which"):
        K.scan(9, U32([1]), U32)
