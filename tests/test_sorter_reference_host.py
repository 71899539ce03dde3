"""CPU checks of what the GPU tests of the suffix sorter compare with (tests/kprobe.py): the numpy references against
plainer ones, the invariants of the active-list generator for every shape the GPU tests build, and -- for four kernels --
that a one-line mutation of the kernel's model trips the assertion the GPU test makes (no broken device code is built)."""
import numpy as np
import pytest

import kprobe as K
import sorter_cases as C
from kprobe import U8, U32, U64


@pytest.mark.parametrize("n", (1, 2, 3, 64, 333, 2000))
def test_reference_suffix_sort_against_sorted_slices(n):
    for name, text in K.text_inputs(n).items():
        code, bits, chars, sigma = K.byte_form(text)
        assert np.array_equal(K.ref_suffix_array(code[text]), K.naive_suffix_array(code[text])), name
        d, code, bits, chars, sigma = K.dict_form(text, phrase=97)
        assert len(d) == n and d[-1] == 0 and bits * chars + 1 <= 64
        assert np.array_equal(K.ref_suffix_array(code[d], terminator=0), K.naive_suffix_array(code[d], terminator=0)), name


def test_input_families():
    t = K.text_inputs(20000)
    assert set(K.PERIODIC_AND_RUNS) <= set(t) and all(len(v) == 20000 for v in t.values())
    assert K.fibonacci_string(13) == "abaababaabaab" and K.thue_morse(8) == "abbabaab"
    runs = "".join(chr(c) for c in t["runs"]).replace("a", "|").replace("c", "|").replace("g", "|").replace("t", "|").split("|")
    assert all(50 <= len(r) <= 5000 for r in runs[:-1]) and len(runs) > 4
    d, code, bits, chars, sigma = K.dict_form(t["runs"])
    assert bits <= 3 and (d == 1).sum() >= 20 and K.ref_run_ends(code[d].tolist(), chars)
    assert K.round_bound(20000, 64) == 10 and K.round_bound(64, 64) == 1 and K.round_bound(4097, 21) == 9


@pytest.mark.parametrize("cap", (1024, 2048))
def test_active_list_generator(cap):
    shapes = K.round_shapes(cap)
    t = cap // 2
    seen = set()
    for name, (sizes, gaps, tail) in shapes.items():
        al = K.ActiveList(sizes, gaps, tail, seed=len(name))
        assert al.check()
        seen |= set(sizes)
        n_tiles = (al.m + t - 1) // t
        bound = K.ref_bounds(al.headc, t, cap, n_tiles)
        ranges = K.ref_ranges(bound, cap)
        # the ranges tile the list, begin and end on bucket boundaries, and only those beyond the capacity are long
        assert ranges[0][2] == 0 and ranges[-1][3] == al.m and all(a[3] == b[2] for a, b in zip(ranges, ranges[1:]))
        starts = set(np.flatnonzero(np.r_[True, al.headc[1:] != al.headc[:-1]]).tolist()) | {al.m}
        assert all(b in starts and e in starts for (_, _, b, e, _) in ranges)
        if name == "four_tiles":
            assert bound[1:4].tolist() == [K.NO_BOUND] * 3
        if name == "ends_at_m":
            assert al.n == int(al.pos[-1]) + 1
        if name == "last_tile_one_bucket":
            assert len(set(al.headc[(n_tiles - 1) * t:].tolist())) == 1 and int(bound[n_tiles - 1]) == (n_tiles - 1) * t
        if name == "many_long":
            assert sum(1 for r in ranges if r[4]) >= 3
        keys, ks, sac_sorted, newhead, flags = K.ref_round(al, 1)
        assert np.all(newhead <= al.pos) and np.all(newhead >= al.headc) and sorted(sac_sorted.tolist()) == sorted(al.sac.tolist())
        assert np.array_equal(ks >> U64(al.shift), al.headc.astype(U64))        # sorting permutes inside buckets only
    assert {2, 128, 129, t - 1, t, t + 1, cap - 1, cap, cap + 1} <= seen


def test_bounds_model_against_a_walk():
    al = K.ActiveList(*K.round_shapes(2048)["cap_edge"][:2], tail=1)
    for target, limit in ((1024, 2048), (512, 1024), (7, 9)):
        n_tiles = (al.m + target - 1) // target
        got = K.ref_bounds(al.headc, target, limit, n_tiles)
        for t in range(1, n_tiles):
            c = t * target
            stop = min(c + limit, al.m)
            while c < stop and al.headc[c] == al.headc[c - 1]:
                c += 1
            assert got[t] == (al.m if c >= al.m else K.NO_BOUND if c == stop else c)


# ---- the GPU tests can fail: a one-line mutation of each kernel's model trips the assertion made on the device's output ----
def test_mutation_short_edge_of_round_fused():
    """SHORT off by one (`cnt < SHORT` in the counting loop, no bitonic fallback for exactly 129): the last member of a
    bucket of 129 is never counted, so two elements take one slot -- the assertions fused_round makes on a tile
    (sorter_cases.check_sorted_tile) pass for the model's output and trip for the mutant's"""
    al = K.ActiveList([129, 2], [0, 0], 0, seed=3)
    keys, ks, sac_sorted, newhead, flags = K.ref_round(al, 1)
    C.check_sorted_tile(ks, sac_sorted, newhead, flags, sac_sorted, newhead, flags, 0, al.m)
    second = keys[:129] & U64((1 << al.shift) - 1)
    slot = np.array([sum(1 for j in range(128) if (second[j], j) < (second[i], i)) for i in range(129)])      # 128, not 129
    r_mut = np.zeros(129, U64); v_mut = np.full(129, K.SENT32, U32)                      # the tile's LDS columns after the scatter
    r_mut[slot] = second; v_mut[slot] = al.sac[:129]
    head_mut = newhead.copy()
    head_mut[:129] = K.ref_running_max(K.ref_mark_subheads(r_mut, al.pos[:129]))
    flags_mut = flags.copy()
    flags_mut[:129] = K.ref_round_flags(head_mut[:129], al.pos[:129])
    sac_mut = sac_sorted.copy()
    sac_mut[:129] = v_mut
    with pytest.raises(AssertionError):
        C.check_sorted_tile(ks, sac_sorted, newhead, flags, sac_mut, head_mut, flags_mut, 0, al.m)


def test_mutation_32_bit_sum_in_make_round_keys():
    """`uint32_t i = sa + h`: for h = 2^32 - sa the sum wraps into the text -- test_round_keys_both_kernels compares with
    a second component of 0"""
    rank = U32(np.arange(50) + 1)
    sac, headc = U32([5, 9]), U32([0, 0])
    h = (1 << 32) - 5
    want = K.ref_round_keys(sac, headc, rank, 50, h, 6)
    mutant = [int(rank[(int(s) + h) & 0xFFFFFFFF]) + 1 if ((int(s) + h) & 0xFFFFFFFF) < 50 else 0 for s in sac]
    assert want.tolist() == [0, 0] and mutant != want.tolist()


def test_mutation_second_sort_call_of_the_tagged_route():
    """dropping the sort by the range tag (end_bit < 32): the elements leave ordered by key across ranges, so a range
    receives elements of another one -- sorter_cases._check_ranges, the assertion of every range-sort test, passes for
    the model of the route and trips for the mutant"""
    rng = np.random.default_rng(1)
    n, end_bit = 60, 3
    kin = U32(rng.integers(0, 8, n)) | (U32(rng.integers(1, 1 << 16, n)) << U32(end_bit))
    vin = U64(rng.permutation(n))
    begin, end = [30, 5], [50, 25]
    off = [0, 20, 40]                                          # the compact array: the ranges by begin, [5, 25) then [30, 50)
    src = np.r_[np.arange(5, 25), np.arange(30, 50)]
    tag = np.repeat([0, 1], 20)
    low = kin[src] & U32((1 << end_bit) - 1)

    def route(order):
        kout = np.full(n, K.SENT32, U32); vout = np.full(n, K.SENT64, U64)
        kout[src] = kin[src][order]; vout[src] = vin[src][order]          # slot c of the sorted array goes back to range slot c
        return kout, vout

    kout, vout = route(np.lexsort((low, tag)))                 # by the low bits, then (stable) by the tag
    C._check_ranges(kin, vin, kout, vout, begin, end, end_bit)
    kout, vout = route(np.argsort(low, kind="stable"))         # the second call dropped
    with pytest.raises(AssertionError):
        C._check_ranges(kin, vin, kout, vout, begin, end, end_bit)


def test_mutation_32_bit_accumulator():
    """exclusive_sum_u32_to_u64 with a 32-bit accumulator: three values of 0xC0000000 give 0x80000000 in the last slot"""
    a = U32([0xC0000000] * 3)
    want = (np.cumsum(a.astype(U64)) - a).tolist()
    mutant = (np.cumsum(a, dtype=U32) - a).astype(U64).tolist()
    assert want == [0, 0xC0000000, 0x180000000] and mutant != want


def test_references_of_first_keys():
    sym = [2, 2, 1, 3, 0]
    assert K.ref_pack_keys(sym, 2, 3).tolist() == [0b101001, 0b100111, 0b011100, 0b110000, 0]
    # separator 1: the window is cut behind it and the low bit says so
    assert K.ref_pack_keys(sym, 2, 3, 1).tolist() == [(0b101001 << 1) | 1, (0b100100 << 1) | 1, (0b010000 << 1) | 1, 0b110000 << 1, 0]
    assert K.ref_pack_keys_u32([5, 6], 3, 2).tolist() == [0b101110, 0b110000]
    assert K.ref_run_ends([1, 1, 1, 2, 0, 0, 0, 3, 3, 3], 3) == [2, 9]
    assert K.ref_mark_heads([4, 4, 5, 7, 7], False).tolist() == [0, 0, 2, 3, 0]
    assert K.ref_mark_heads([4, 4, 5, 7, 7], True).tolist() == [0, 0, 2, 3, 4]
    assert K.ref_flag_unsorted([0, 0, 2, 3, 3]).tolist() == [1, 1, 0, 1, 1]
    assert K.ref_equal_range([1, 3, 3, 9], [3, 4]).tolist() == [1, 3, 3, 3]
