"""The cases of tests/test_gpu_sorter_kernels.py and tests/test_gpu_sorter_forms.py that depend on a switch read once per
process (MMT_ROUND_CAP, MMT_GIANT_RANGE, MMT_RANGES_AS_ONE, MMT_SORT_FUSED, MMT_BIG_CAP, MMT_SORT_GLOBAL_ROUNDS): plain
functions, run in-process for the default setting and by `python sorter_cases.py GROUP` in a child process for any other
(one child runs all cases of one setting and prints "sorter cases ok: N")."""
import os
import sys

import numpy as np

import kprobe as K
from kprobe import U8, U32, U64, SENT8, SENT32, SENT64, NO_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# one doubling round, kernel by kernel: every stage is compared with the model and fed the model's values
# ---------------------------------------------------------------------------------------------------------------------
def _big_list_ok(begin, end, count, big_cap, want):
    """the list of long ranges: all counted, the first min(count, cap) slots distinct members of `want`, the rest untouched"""
    assert count == len(want), (count, len(want))
    k = min(count, big_cap)
    got = list(zip(begin[:k].tolist(), end[:k].tolist()))
    assert len(set(got)) == k and set(got) <= set(want), (got, want)
    if count <= big_cap:
        assert set(got) == set(want)
    assert np.all(begin[k:] == SENT32) and np.all(end[k:] == SENT32), "a slot beyond the capacity was written"


def check_sorted_tile(ks, sac_sorted, newhead, flags_want, sac_out, head_out, flags, b, e):
    """what round_fused must leave for a range [b, e) that fits a tile: heads and flags exactly, suffixes as sets per run of equal keys"""
    assert np.array_equal(head_out[b:e], newhead[b:e]), ("heads", b, e)
    assert np.array_equal(flags[b:e], flags_want[b:e]), ("flags", b, e)
    assert K.same_sets_per_run(ks, sac_out, sac_sorted, b, e), ("suffixes", b, e)


def fused_round(al, h, cap, big_cap_delta):
    """round_head_bounds + round_fused + round_big_keys + range sort + round_big_subheads + running maximum +
    round_big_apply; big_cap = number of long ranges + big_cap_delta.  Returns (heads, flags) of the round."""
    assert cap == K.lib().kp_round_fused_cap()
    m, n, shift = al.m, al.n, al.shift
    target, limit = cap // 2, cap
    n_tiles = (m + target - 1) // target
    keys, ks, sac_sorted, newhead, flags_want = K.ref_round(al, h)
    bound_want = K.ref_bounds(al.headc, target, limit, n_tiles)
    bound = np.empty(n_tiles + 1, U32)
    K.call("round_head_bounds", al.headc, m, target, limit, n_tiles, bound)
    assert np.array_equal(bound, bound_want), "round_head_bounds"
    ranges = K.ref_ranges(bound_want, cap)
    longs = [(b, e) for (_, _, b, e, lg) in ranges if lg]
    big_cap = len(longs) + big_cap_delta          # (0: a legal list that holds nothing; round_cases asks for no negative one)
    assert big_cap >= 0
    alloc = big_cap + 4
    sa = np.full(n, SENT32, U32); sac_out = np.full(m, SENT32, U32); head_out = np.full(m, SENT32, U32)
    flags = np.full(m, SENT8, U8); bb = np.full(alloc, SENT32, U32); be = np.full(alloc, SENT32, U32)
    cnt = np.zeros(1, U32); tile_big = np.zeros(n_tiles + 1, U8)
    K.call("round_fused", al.sac, al.headc, al.pos, m, bound_want, n_tiles, al.rank, n, K.c_u32(h), shift, sa, sac_out, head_out,
           flags, bb, be, alloc, cnt, big_cap, tile_big)
    _big_list_ok(bb, be, int(cnt[0]), big_cap, longs)
    assert np.array_equal(tile_big, K.ref_tile_big(bound_want, cap)), "tile marks"
    inactive = np.ones(n, bool); inactive[al.pos] = False
    assert np.all(sa[inactive] == SENT32), "round_fused wrote a suffix-array entry outside the active list"
    for (_, _, b, e, lg) in ranges:
        if lg:
            assert np.all(sac_out[b:e] == SENT32) and np.all(head_out[b:e] == SENT32) and np.all(flags[b:e] == SENT8)
            assert np.all(sa[al.pos[b:e]] == SENT32)
        else:
            check_sorted_tile(ks, sac_sorted, newhead, flags_want, sac_out, head_out, flags, b, e)
            assert np.array_equal(sa[al.pos[b:e]], sac_out[b:e]), ("SA[pos]", b, e)
    if int(cnt[0]) > big_cap:
        return None                                    # (sorter.cpp falls back to the round of separate kernels)
    if longs:
        marks = K.ref_tile_big(bound_want, cap)
        kbig = np.full(m, SENT64, U64)
        K.call("round_big_keys", marks, bound_want, target, n_tiles, al.sac, al.headc, m, al.rank, n, n, K.c_u32(h), shift, kbig)
        in_long = np.zeros(m, bool)
        for b, e in longs:
            in_long[b:e] = True
        assert np.array_equal(kbig[in_long], keys[in_long]) and np.all(kbig[~in_long] == SENT64), "round_big_keys"
        kout, vout = K.sort_ranges(keys, al.sac, [b for b, _ in longs], [e for _, e in longs], min(64, 2 * shift), ordered=True)
        for b, e in longs:
            assert np.array_equal(kout[b:e], ks[b:e]) and K.same_sets_per_run(ks, vout, sac_sorted, b, e), ("range sort", b, e)
        assert np.all(kout[~in_long] == SENT64) and np.all(vout[~in_long] == SENT32)
        head_io = head_out.copy()
        K.call("round_big_subheads", marks, bound_want, target, n_tiles, np.where(in_long, ks, U64(SENT64)), al.pos, m, head_io)
        assert np.array_equal(head_io[in_long], K.ref_mark_subheads(ks, al.pos)[in_long]), "round_big_subheads"
        # (the first element of a long range is a head whatever stands in front of it)
        assert np.array_equal(head_io[~in_long], head_out[~in_long])
        head_all = K.scan(0, head_io, U32)
        assert np.array_equal(head_all, newhead), "running maximum over the head column"
        K.call("round_big_apply", marks, bound_want, target, n_tiles, m, np.where(in_long, vout, U32(SENT32)), newhead, al.pos,
               sa, n, flags)
        sac_out = np.where(in_long, vout, sac_out)
        head_out = head_all
    assert np.array_equal(head_out, newhead) and np.array_equal(flags, flags_want)
    assert np.array_equal(sa[al.pos], sac_out) and np.all(sa[inactive] == SENT32)
    assert K.same_sets_per_run(ks, sac_out, sac_sorted)
    return head_out, flags


def tiled_round(al, h, big_cap_delta, high_heads=False):
    """make_round_keys + round_tile_bounds + round_local_sort + range sort + mark_subheads + running maximum +
    apply_round.  high_heads: the key-only kernels once more with heads beyond 2^31 at shift 32."""
    m, n = al.m, al.n
    cap, target = int(K.lib().kp_round_tile_cap()), 1024
    n_tiles = (m + target - 1) // target
    shift = 32 if high_heads else al.shift
    headc = (al.headc.astype(U64) + U64(0x80000000 if n < 0x40000000 else 0)).astype(U32) if high_heads else al.headc
    if high_heads:
        headc[len(headc) // 2:] |= U32(0x40000000)            # bits 62 and 63 of the keys
    keys = np.empty(m, U64)
    K.call("make_round_keys", al.sac, headc, m, al.rank, n, n, K.c_u32(h), shift, keys)
    keys_want = K.ref_round_keys(al.sac, headc, al.rank, n, h, shift)
    assert np.array_equal(keys, keys_want), "make_round_keys"
    order = np.argsort(keys_want, kind="stable")
    ks, sac_sorted = keys_want[order], al.sac[order]
    bound_want = K.ref_bounds(headc, target, cap, n_tiles)
    bound = np.empty(n_tiles + 1, U32)
    K.call("round_tile_bounds", keys_want, m, shift, target, cap, n_tiles, bound)
    assert np.array_equal(bound, bound_want), "round_tile_bounds"
    ranges = K.ref_ranges(bound_want, cap)
    longs = [(b, e) for (_, _, b, e, lg) in ranges if lg]
    big_cap = len(longs) + big_cap_delta          # (0: a legal list that holds nothing; round_cases asks for no negative one)
    assert big_cap >= 0
    alloc = big_cap + 4
    kout = np.full(m, SENT64, U64); vout = np.full(m, SENT32, U32)
    bb = np.full(alloc, SENT32, U32); be = np.full(alloc, SENT32, U32); cnt = np.zeros(1, U32)
    K.call("round_local_sort", keys_want, al.sac, m, bound_want, n_tiles, kout, vout, bb, be, alloc, cnt, big_cap, shift)
    _big_list_ok(bb, be, int(cnt[0]), big_cap, longs)
    for (_, _, b, e, lg) in ranges:
        if lg:
            assert np.all(kout[b:e] == SENT64) and np.all(vout[b:e] == SENT32)
        else:
            assert np.array_equal(kout[b:e], ks[b:e]), ("keys", b, e)
            assert K.same_sets_per_run(ks, vout, sac_sorted, b, e), ("suffixes", b, e)
    if int(cnt[0]) > big_cap or high_heads:
        return None
    if longs:
        k2, v2 = K.sort_ranges(keys_want, al.sac, [b for b, _ in longs], [e for _, e in longs], min(64, 2 * shift), ordered=True)
        for b, e in longs:
            assert np.array_equal(k2[b:e], ks[b:e]) and K.same_sets_per_run(ks, v2, sac_sorted, b, e)
            kout[b:e] = k2[b:e]; vout[b:e] = v2[b:e]
    assert np.array_equal(kout, ks)
    headval = np.empty(m, U32)
    K.call("mark_subheads", ks, al.pos, m, headval)
    assert np.array_equal(headval, K.ref_mark_subheads(ks, al.pos)), "mark_subheads"
    newhead = K.scan(0, headval, U32)
    assert np.array_equal(newhead, K.ref_running_max(headval))
    sa = np.full(n, SENT32, U32); rank = al.rank.copy(); flags = np.empty(m, U8)
    K.call("apply_round", vout, newhead, al.pos, m, sa, rank, n, flags)
    want_rank = al.rank.copy(); want_rank[vout] = newhead
    inactive = np.ones(n, bool); inactive[al.pos] = False
    assert np.array_equal(sa[al.pos], vout) and np.all(sa[inactive] == SENT32), "apply_round: SA"
    assert np.array_equal(rank, want_rank), "apply_round: rank"
    assert np.array_equal(flags, K.ref_round_flags(newhead, al.pos)), "apply_round: flags"
    return newhead, flags


def round_cases():
    """every bucket shape, both forms of the round, the three capacities of the long-range list; the forms agree"""
    cap = int(K.lib().kp_round_fused_cap())
    done = 0
    for name, (sizes, gaps, tail) in K.round_shapes(cap).items():
        al = K.ActiveList(sizes, gaps, tail, seed=len(name))
        al.check()
        for h in (1, max(1, al.n // 5)):
            full_f = fused_round(al, h, cap, 3)
            full_t = tiled_round(al, h, 3)
            assert full_f is not None and full_t is not None
            assert np.array_equal(full_f[0], full_t[0]) and np.array_equal(full_f[1], full_t[1]), name
            done += 2
        # the list of long ranges exactly full, and one slot short (where there is a long range to leave out)
        n_long = {form: sum(1 for r in K.ref_ranges(K.ref_bounds(al.headc, c // 2, c, (al.m + c // 2 - 1) // (c // 2)), c) if r[4])
                  for form, c in (("fused", cap), ("tiled", int(K.lib().kp_round_tile_cap())))}
        for delta in (0, -1):
            if n_long["fused"] + delta >= 0:
                fused_round(al, 1, cap, delta); done += 1
            if n_long["tiled"] + delta >= 0:
                tiled_round(al, 1, delta); done += 1
        tiled_round(al, 1, 3, high_heads=True)
        done += 1
    return done


# ---------------------------------------------------------------------------------------------------------------------
# the range sorts
# ---------------------------------------------------------------------------------------------------------------------
def _check_ranges(kin, vin, kout, vout, begin, end, end_bit):
    kbits = kin.itemsize * 8
    mask = (1 << min(end_bit, kbits)) - 1
    touched = np.zeros(len(kin), bool)
    for b, e in zip(begin, end):
        touched[b:e] = True
        mk = np.array([int(x) & mask for x in kin[b:e]], dtype=object)
        order = sorted(range(e - b), key=lambda i: mk[i])
        want_m = [mk[i] for i in order]
        got_m = [int(x) & mask for x in kout[b:e]]
        assert got_m == want_m, ("keys of range", b, e)
        want_pairs = [(int(kin[b + i]), int(vin[b + i])) for i in order]
        got_pairs = [(int(kout[c]), int(vout[c])) for c in range(b, e)]
        c = 0
        while c < e - b:
            d = c
            while d + 1 < e - b and want_m[d + 1] == want_m[c]:
                d += 1
            assert sorted(got_pairs[c:d + 1]) == sorted(want_pairs[c:d + 1]), ("pairs of range", b, e)
            c = d + 1
    sk = SENT64 if kin.itemsize == 8 else SENT32
    sv = SENT64 if vin.itemsize == 8 else SENT32
    assert np.all(kout[~touched] == sk) and np.all(vout[~touched] == sv), "an element outside the ranges was touched"


def range_lists(n, long_len):
    """name -> (begin, end) inside [0, n): the list shapes of the issue; long_len: the length of the longest range"""
    assert n >= long_len + 400
    L = long_len
    return {
        "single": ([7], [7 + L]),
        "empty_among": ([3, 60, 60, 100 + L + 9], [40, 60, 100 + L, 100 + L + 9]),
        "adjacent": ([0, 50, 50 + L], [50, 50 + L, 50 + L + 90]),
        "out_of_order": ([200 + L, 5, 120], [260 + L, 70, 120 + L]),
        "gaps": ([10, 100, 200 + L], [33, 100 + L, 300 + L]),
    }


def range_cases(long_len):
    """all four type pairs through every list shape; which route runs is decided by the process's switches and by
    long_len (see prims.hip, sort_ranges): the caller picks both"""
    rng = np.random.default_rng(long_len)
    n = long_len + 500
    done = 0
    for kd, vd in ((U32, U32), (U32, U64), (U64, U32), (U64, U64)):
        for name, (begin, end) in range_lists(n, long_len).items():
            vin = (rng.integers(0, 1 << 31, n).astype(vd) << (vd(29) if vd == U64 else vd(0))) | np.arange(n).astype(vd)
            for end_bit in ((32, 13) if kd == U32 else (64, 40)):
                # few distinct values below end_bit (ties), garbage above it when it is below the key's width
                kin = rng.integers(0, 50, n).astype(kd) << kd(max(0, min(end_bit, 40) - 6))
                if end_bit < kd(0).itemsize * 8:
                    kin |= rng.integers(1, 1 << 16, n).astype(kd) << kd(end_bit)
                elif kd == U64:
                    kin |= rng.integers(0, 4, n).astype(kd) << kd(62)           # bits 62 and 63
                kout, vout = K.sort_ranges(kin, vin, begin, end, end_bit)
                _check_ranges(kin, vin, kout, vout, begin, end, end_bit)
                done += 1
            if kd == U64 and vd == U32:
                # keys that order the ranges (the bucket in the high bits, bits 62 and 63 among them): all ranges as one sort
                rank_of = np.argsort(np.argsort(begin))
                kin = rng.integers(0, 40, n).astype(U64)
                for r, (b, e) in enumerate(zip(begin, end)):
                    kin[b:e] |= U64(int(rank_of[r]) + 11) << U64(60)
                kout, vout = K.sort_ranges(kin, vin, begin, end, 64, ordered=True)
                _check_ranges(kin, vin, kout, vout, begin, end, 64)
                # the same range twice overlaps itself: the as-one route declines, the route behind it sorts the range
                kin2 = u64_distinct(rng, n)
                kout, vout = K.sort_ranges(kin2, vin, [begin[0], begin[0]], [end[0], end[0]], 64, ordered=True)
                _check_ranges(kin2, vin, kout, vout, [begin[0]], [end[0]], 64)
                done += 2
    return done


def u64_distinct(rng, n):
    return (rng.integers(0, 1 << 40, n).astype(U64) << U64(23)) | rng.permutation(n).astype(U64)


# ---------------------------------------------------------------------------------------------------------------------
# the sorter in its three call forms
# ---------------------------------------------------------------------------------------------------------------------
def _check_sort(sa, rank, rounds, want, n, h0, what):
    assert np.array_equal(sa, want), what + ": suffix array"
    inv = np.empty(n, U32); inv[want] = np.arange(n, dtype=U32)
    assert np.array_equal(rank, inv), what + ": rank is not the inverse"
    assert rounds <= K.round_bound(n, h0), (what, rounds, K.round_bound(n, h0))


def form_cases(sizes, names=None):
    """byte-text, dictionary (with and without RunRefine) and integer form on every input; returns the suffix arrays
    (name, n, form) -> sa so that processes with different switches can be compared"""
    out = {}
    for n in sizes:
        for name, text in K.text_inputs(n).items():
            if names and name not in names:
                continue
            code, bits, chars, sigma = K.byte_form(text)
            sa, rank, rounds, _ = K.sorter_text(text, code, bits, chars, sigma)
            _check_sort(sa, rank, rounds, K.ref_suffix_array(code[text]), n, chars, "%s %d text" % (name, n))
            out[(name, n, "text")] = sa
            d, code, bits, chars, sigma = K.dict_form(text)
            assert bits <= 3, "RunRefine takes symbols of three bits at the most: every input must get its RunRefine case"
            want = K.ref_suffix_array(code[d], terminator=0)
            for use_runs in (False, True):
                # MMT_RUN_BUCKET is read at every call: 2 for this one sort, then as it was
                with K.environment(MMT_RUN_BUCKET="2"):
                    sa, rank, rounds, refined = K.sorter_text(d, code, bits, chars, sigma, sep_code=int(code[1]), use_runs=use_runs)
                _check_sort(sa, rank, rounds, want, n, chars, "%s %d dict runs=%d" % (name, n, use_runs))
                if name == "a^n" and 4095 <= n <= 4097:
                    # the bucket a^chars holds fewer suffixes than the default threshold of 4096: only the lowered one refines it
                    bucket = int(np.sum(K.ref_pack_keys(code[d], bits, chars, int(code[1])) == np.uint64(((1 << bits * chars) - 1) // ((1 << bits) - 1) * int(code[97]) << 1)))
                    assert 2 <= bucket < 4096 and refined == (bucket if use_runs else 0), (bucket, refined)
                out[(name, n, "dict%d" % use_runs)] = sa
            sym = code_ints(text)
            ibits, ichars = K.int_form(sym)
            sa, rank, rounds = K.sorter_ints(sym, ibits, ichars)
            _check_sort(sa, rank, rounds, K.ref_suffix_array(sym), n, ichars, "%s %d ints" % (name, n))
            out[(name, n, "ints")] = sa
        if names is None:
            # an alphabet of 2^20 symbols with one symbol repeated thousands of times
            rng = np.random.default_rng(n)
            sym = rng.integers(1, (1 << 20) + 1, n).astype(U32)
            sym[rng.random(n) < 0.4] = 77777
            sym[n // 3: n // 3 + min(n // 4, 3000)] = 77777
            if n:
                sym[-1] = 1 << 20
            ibits, ichars = K.int_form(sym)
            assert (ibits, ichars) == (21, 3) or n < 1
            sa, rank, rounds = K.sorter_ints(sym, ibits, ichars)
            _check_sort(sa, rank, rounds, K.ref_suffix_array(sym), n, ichars, "alphabet 2^20, n %d" % n)
            out[("big_alphabet", n, "ints")] = sa
    return out


def code_ints(text):
    """the letters of a text as parse symbols 1 .. D spread over 17 bits (key_bits differs from a byte text's)"""
    return (text.astype(U32) - U32(64)) * U32(1031)


def sa_digest(out):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(repr(k).encode()); h.update(out[k].tobytes())
    return h.hexdigest()


GROUPS = {
    "round": lambda: round_cases(),
    "ranges_small": lambda: range_cases(300),
    "forms_switch": lambda: len(form_cases((4097, 20000), K.PERIODIC_AND_RUNS)),
}

if __name__ == "__main__":
    total = 0
    for g in sys.argv[1:]:
        if g == "forms_digest":
            print("sa digest", sa_digest(form_cases((4097, 20000), K.PERIODIC_AND_RUNS)))
            total += 1
        else:
            total += GROUPS[g]()
    print("sorter cases ok: %d" % total)
