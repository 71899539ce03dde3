"""The kernels of the prefix-free parse one by one (csrc/pfp_kernels.hip rows A2-A4, the dictionary's LCP steps of csrc/kernels.hip,
csrc/parse_lcp.hip): every launch wrapper through the probe library (tests/kprobe) against the plain model tests/pfpmodel.py,
on the inputs of tests/pfp_cases.py -- the boundaries of every path chosen by shape, and forged inputs for the code no real
input reaches (fingerprint collisions, saturation, overflow guards).  Every comparison is exact, every in/out array carries
sentinels behind what the wrapper may write.  tests/test_pfp_model_host.py holds the model and the checks themselves."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kprobe as K
import pfp_cases as C
import pfpmodel as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64


# ---- triggers ---------------------------------------------------------------------------------------------------------------------
def _trigger_window(w, plain):
    """every length, text and modulus for one window: bytes aligned (and with MMT_TRIGGER_PLAIN when `plain`), bytes with
    misalign 1 and 15 (the wrapper's fall-back to the generic kernel), packed"""
    ran = 0
    for n in C.trigger_lengths(w):
        for name, text in C.trigger_texts(n, w).items():
            hashes = P.kr_hashes(text, w)
            forms = [("bytes", K.Text(text))]
            if not plain:
                forms += [("misalign 1", K.Text(text, misalign=1)), ("misalign 15", K.Text(text, misalign=15)),
                          ("packed", K.Text(text, "packed"))]
            for p in C.TRIGGER_MODULI:
                cuts = P.triggers(text, w, p, hashes)
                for form, tx in forms:
                    masks, counts = K.trigger_masks(tx, w, p)
                    C.check_trigger_masks(masks, counts, n, w, cuts, "w %d p %d n %d %s %s%s" % (w, p, n, name, form, " plain" if plain else ""))
                    ran += 1
    return ran


@pytest.mark.parametrize("w", C.FAST_WINDOWS + C.GENERIC_WINDOWS)
def test_trigger_masks(w):
    assert _trigger_window(w, False) == len(C.trigger_lengths(w)) * 3 * len(C.TRIGGER_MODULI) * 4


def test_trigger_masks_plain_switch():
    """MMT_TRIGGER_PLAIN is a live switch: set around the calls, the generic kernel serves the aligned byte text too.  (Were
    the probe's copy of the switch table to read it only once, this process would already have run without it: the child
    below then is the one that runs the plain kernel.)"""
    with K.environment(MMT_TRIGGER_PLAIN="1"):
        for w in (4, 10, 16):
            _trigger_window(w, True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "plain"], env=dict(os.environ, MMT_TRIGGER_PLAIN="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plain triggers ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_trigger_blocks():
    for n in (1, 16, 4096, 4097, 8193, 1 << 33):
        assert K.trigger_blocks(n) == P.trigger_blocks(n)


@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("kind", C.CUT_KINDS)
def test_trigger_cuts(kind, wide):
    n = C.CUT_N
    masks = C.forged_masks(n, kind)
    _, counts = P.trigger_masks(n, P.cuts_of_masks(masks, n))
    off = np.cumsum(counts.astype(np.int64)) - counts
    total = int(counts.astype(np.int64).sum())
    cuts = K.trigger_cuts(masks, n, off, total + 2, wide)
    C.check_cuts(cuts, masks, n, "%s wide %d" % (kind, wide))


def test_phrase_bounds():
    for wide in (False, True):
        for cuts, n, w in (([], 50, 10), ([9, 10, 11, 12, 40], 50, 10), ([3, 4, 5], 6, 4), (list(range(20, 600, 2)), 700, 6)):
            start, length = K.phrase_bounds(cuts, n, w, wide)
            ws, wl = P.phrase_bounds(cuts, n, w)
            C.column(start, np.asarray(ws, dtype=start.dtype), "start"); C.column(length, K.u32(wl), "len")
    big = (1 << 32) + (1 << 31) + 5                            # wide: no text is read, the cut values are forged above 2^32
    cuts = [(1 << 32) - 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) + (1 << 31)]       # (every phrase below 2^32 characters)
    start, length = K.phrase_bounds(cuts, big, 10, True)
    ws, wl = P.phrase_bounds(cuts, big, 10)
    C.column(start, K.u64(ws), "wide start"); C.column(length, K.u32(wl), "wide len")


# ---- fingerprints -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("bytes", "packed"))
def test_phrase_hash(layout):
    for name, (text, start, lens) in C.hash_cases().items():
        tx = K.Text(text, layout)
        for wide in (False, True):
            h1, pinfo = K.phrase_hash(tx, start, lens, wide)
            C.check_phrase_hash(h1, pinfo, tx.v, start, lens, "%s %s wide %d" % (name, layout, wide))


@pytest.mark.parametrize("layout", ("bytes", "packed"))
def test_phrase_hash_routes_agree(layout):
    (text, start, lens), idx = C.route_case()
    tx = K.Text(text, layout)
    h1, pinfo = K.phrase_hash(tx, start, lens)
    C.check_phrase_hash(h1, pinfo, tx.v, start, lens, "routes")
    C.check_same_fingerprint(h1, pinfo, idx, "routes " + layout)


def test_second_fingerprint():
    rng = np.random.default_rng(2)
    for m in (1, 255, 256, 257):
        pinfo = rng.integers(0, 1 << 32, (m, 4), dtype=np.int64).astype(U32)
        pinfo[:, 1] |= U32(0xFF000000)                         # the start's high byte rides in the top byte: not part of h2
        C.column(K.second_fingerprint(pinfo), P.second_fingerprint(pinfo), "h2 m %d" % m)


# ---- distinct phrases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("bytes", "packed"))
@pytest.mark.parametrize("name", ("runs", "collide", "h1_only"))
def test_mark_distinct(name, layout):
    text, order, h1s, pinfo = C.distinct_cases()[name]
    tx = K.Text(text, layout)
    flags, err = K.mark_distinct(order, h1s, pinfo, tx)
    C.check_mark_distinct(flags, err, tx.v, order, h1s, pinfo, name + " " + layout)


def test_assign_distinct():
    rng = np.random.default_rng(3)
    for m in (1, 2, 256, 257, 700):
        order = rng.permutation(m).astype(U32)
        flags = (rng.random(m) < 0.3).astype(U32); flags[0] = 1
        length = rng.integers(1, 5000, m).astype(U32)
        scan, pid, rep, dlen = P.assign_distinct(order, flags, length)
        d = len(rep)
        gp, gr, gd = K.assign_distinct(order, scan, flags, length, d + 2)
        C.same(gp, pid, "pid"); C.column(gr, rep, "rep"); C.column(gd, dlen, "dlen")


def test_sum_u32():
    assert K.sum_u32([]) == 0
    assert K.sum_u32([0xFFFFFFFF] * 3) == 3 * 0xFFFFFFFF       # beyond 2^32
    x = np.random.default_rng(4).integers(0, 1 << 32, 257, dtype=np.int64)
    assert K.sum_u32(x) == int(x.sum())
    x = np.random.default_rng(5).integers(0, 1 << 32, 300000, dtype=np.int64)      # more than one pass of the grid
    assert K.sum_u32(x) == int(x.sum())


# ---- dictionary ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("bytes", "packed"))
def test_copy_dict(layout):
    text, start, lens, which, dstart, nd = C.copy_case()
    tx = K.Text(text, layout)
    for wide in (False, True):
        for pack_prev in (True, False):
            d, info = K.copy_dict(tx, start, lens, which, dstart, nd, pack_prev, wide)
            C.check_copy_dict(d, info, tx.v, start, lens, which, dstart, nd, pack_prev, None, "pack %d wide %d" % (pack_prev, wide))
    d, info = K.copy_dict(tx, start, lens, which, dstart, nd, True, with_info=False)
    C.check_copy_dict(d, None, tx.v, start, lens, which, dstart, nd, True, None, "dinfo null")
    bad = list(dstart); bad[3] = nd - lens[which[3]]           # o + l = dict_len: the guard refuses the phrase
    d, info = K.copy_dict(tx, start, lens, which, bad, nd, True)
    C.check_copy_dict(d, info, tx.v, start, lens, which, bad, nd, True, (3, dstart), "guard")


@pytest.mark.parametrize("nd", C.ENTRY_ND)
def test_entry_info(nd):
    d, info, sa_d = C.entry_case(nd)
    for pack_prev in (True, False):
        esuf, ephr, ebw = K.entry_info(sa_d, info, d, pack_prev)
        C.check_entry_info(esuf, ephr, ebw, sa_d, d, info, pack_prev, "nd %d pack %d" % (nd, pack_prev))


def test_dictionary_lcp_chain():
    """dict_irreducible -> long_lcp_lim -> plcp_running_max -> lcp_gather -> dict_lcp_clamp, each stage fed from the model"""
    d, sa_d, esuf, ebw = C.lcp_dictionary()
    first, want_longs, full = P.dict_irreducible(d, sa_d, esuf, ebw)
    assert len(want_longs) >= 3
    for long_cap in (len(want_longs) + 3, 2):                  # 2: fewer slots than long pairs
        plcp, longs, count = K.dict_irreducible(d, sa_d, esuf, ebw, long_cap, len(want_longs) + 5)
        C.check_dict_irreducible(plcp, longs, count, long_cap, d, sa_d, esuf, ebw, "long_cap %d" % long_cap)
    C.same(K.long_lcp_lim(d, sorted(want_longs), first), full, "long_lcp_lim")
    C.column(K.plcp_running_max(full), P.plcp_running_max(full), "plcp_running_max")
    plcp = P.plcp_running_max(full)
    C.column(K.lcp_gather(plcp, sa_d), plcp[sa_d], "lcp_gather")
    lcp = K.dict_lcp_clamp(plcp[sa_d], esuf)
    C.check_dict_lcp(lcp, d, sa_d, esuf, "chain")


# ---- group tables, ranks ----------------------------------------------------------------------------------------------------------------
def test_group_flags():
    esuf, lcp = C.group_case()
    g, p, v, seg = K.group_flags(esuf, lcp, C.GROUP_W)
    C.check_group_flags(g, p, v, seg, esuf, lcp, C.GROUP_W)


@pytest.fixture(scope="module")
def small_model():
    from mumemto_amd import synth
    docs = synth.pangenome(3, 1200, 0.02, seed=21, n_run=(1, 300, 380))
    text = np.frombuffer(b"$".join(d[0] for d in docs) + b"$", U8)
    return P.Model(text, 4, 11)


def test_rank_permutations(small_model):
    M = small_model
    C.column(K.phrase_ranks(M.esuf, M.ephr, M.pscan, M.D + 2), M.prank, "prank")
    C.column(K.parse_ranks(M.pid, M.prank), M.parse, "parse")
    which, slen = K.invert_ranks(M.prank, M.rep, M.dlen)
    C.column(which, M.which, "which"); C.column(slen, M.slen, "slen")
    assert sorted(M.prank.tolist()) == list(range(1, M.D + 1))


# ---- inverted lists -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("m", C.OCC_M)
def test_inverted_lists(m, wide):
    ranks = set()
    for first in (0, 1, 2):
        pid, sa_p, pstart, sl, D, pos_bits = C.occ_case(m, first, wide)
        ranks.add(int(np.flatnonzero(sa_p == 0)[0]))
        keys, vals = K.occ_sequence(sa_p, pid, D)
        C.check_occ_sequence(keys, vals, sa_p, pid, D, "m %d" % m)
        wk, wv = P.occ_sequence(sa_p, pid, D)
        o = np.argsort(wk, kind="stable")
        ids, ts = wk[o], wv[o]
        for mode in (8, 12):
            occ_start, occ, occ_sl = K.occ_finish(mode, ids, ts, sa_p, pstart, wide, sl, pos_bits, D + 2)
            C.check_occ_finish(mode, occ_start, occ, occ_sl, ids, ts, sa_p, pstart, sl, pos_bits, "m %d mode %d wide %d" % (m, mode, wide))
    assert m < 3 or len(ranks) == 3                             # the parse's first suffix sat at several ranks


def test_emitter_inputs(small_model):
    M = small_model
    tab = K.phrase_table(M.occ_start, M.plen, M.rep)
    C.same(tab[:M.D], M.tab, "tab"); C.untouched(tab, M.D, "tab")
    ce = K.entry_compact(M.esuf, M.ephr, M.ebw, M.gflag, M.gscan, M.vflag, M.vscan, M.segmin, M.tab, M.E)
    for k in ce:
        C.column(ce[k], M.ce[k], "ce_" + k)                    # (compact arrays sized exactly: the sentinel sits right behind entry E)
    gh = K.group_heads(M.sege, M.ce["hl"], M.ce["slen"])
    C.same(gh[:M.G], M.ghead, "ghead"); C.untouched(gh, M.G, "ghead")
    assert int(gh[0][1]) == 0
    # the clamp by the shorter neighbour, forged: LCP 9 between suffixes of 4 and 7 characters
    gh = K.group_heads([0, 1, 2], [0, 9, 9], [7, 4, 7])
    C.same(gh[:3], K.u32([[7, 0], [4, 4], [7, 4]]), "forged ghead")


# ---- emitter bookkeeping ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", (False, True))
def test_tile_first(wide):
    tile = K.emit_tile()
    segb, tile_base = C.tile_case(tile, wide)
    tiles = tile_base + 7
    out = K.tile_first(segb, tiles, wide, tile_base)
    C.column(out, P.tile_first(segb, tiles, tile, tile_base), "tile_first")
    if wide:                                                   # a table that begins behind the first groups' tiles
        out = K.tile_first(segb, tiles, wide, tile_base + 1)
        C.column(out, P.tile_first(segb, tiles, tile, tile_base + 1), "tile_first with a later base")


@pytest.mark.parametrize("wide", (False, True))
def test_oversize_and_gathers(wide):
    segb = C.oversize_case(wide)
    osize, err = K.oversize(segb, wide)
    C.check_oversize(osize, err, segb, "wide %d" % wide)
    rng = np.random.default_rng(6)
    src = rng.integers(0, 1 << (40 if wide else 32), 500, dtype=np.int64)
    idx = rng.integers(0, 500, 300)
    out = K.gather_pos(src, idx, wide)
    C.column(out, src[idx].astype(out.dtype), "gather_pos")
    off = np.cumsum(rng.integers(0, 5000, 40)) + ((1 << 33) if wide else (1 << 31))
    for f0, count in ((0, 39), (7, 0), (12, 20)):
        rel = K.relative_offsets(off, f0, count, wide)
        C.column(rel, (off[f0:f0 + count + 1] - off[f0]).astype(U32), "relative_offsets")


def test_iota_and_gather_u64():
    for n in (1, 255, 256, 257, 1000):
        C.column(K.iota(n), np.arange(n, dtype=U32), "iota %d" % n)
    rng = np.random.default_rng(7)
    src = rng.integers(0, 1 << 63, 400, dtype=np.int64).astype(U64) | U64(1 << 63)
    idx = rng.integers(0, 400, 257)
    C.column(K.gather_u64(src, idx), src[idx], "gather_u64")


# ---- parse LCP ----------------------------------------------------------------------------------------------------------------------------
def _parse_lcp(M, what):
    for layout, wide in (("bytes", False), ("bytes", True), ("packed", False)):
        tx = K.Text(M.text, layout)
        sl, bmin, nb, levels, n_irr, n_long = K.parse_lcp(tx, M.nv, M.sa_p, M.pid, M.pstart, wide)
        C.check_parse_lcp(sl, bmin, nb, levels, n_irr, n_long, M, "%s %s wide %d" % (what, layout, wide))


@pytest.mark.parametrize("m", C.PARSE_M)
def test_parse_lcp_sizes(m):
    M = P.Model(C.text_of_m_phrases(m, C.PARSE_W, C.PARSE_P), C.PARSE_W, C.PARSE_P)
    assert M.m == m
    _parse_lcp(M, "m %d" % m)


def test_parse_lcp_shared_lengths():
    M = P.Model(C.shared_text(), C.PARSE_W, C.PARSE_P)
    assert set(C.PARSE_SHARED) <= set(M.sl.tolist()) and M.n_long > 0
    _parse_lcp(M, "shared")


def test_parse_lcp_identical_haplotypes():
    M = P.Model(C.identical_haplotypes(), C.PARSE_W, C.PARSE_P)
    assert M.n_long > 0 and M.n_irreducible < M.m // 2          # long reducible chains
    _parse_lcp(M, "identical")


# ---- RMQ ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", C.RMQ_BUILD_M)
def test_build_rmq(m):
    vals = np.random.default_rng(m).integers(0, 1 << 32, m, dtype=np.int64).astype(U32)
    nb, levels, bmin = K.build_rmq(vals)
    C.check_build_rmq(nb, levels, bmin, vals, "m %d" % m)


def test_rmq_every_pair():
    vals = np.random.default_rng(8).integers(0, 1000, 300).astype(U32)
    pairs = C.rmq_pairs_all(300)
    out, out8 = K.rmq_query(vals, pairs)
    C.check_rmq(out, out8, vals, pairs, "m 300")


def test_rmq_edges_and_minimum_places():
    m = 10000
    pairs = C.rmq_pairs_edges(m)
    vals = np.random.default_rng(9).integers(1000, 1 << 32, m, dtype=np.int64).astype(U32)
    out, out8 = K.rmq_query(vals, pairs)
    C.check_rmq(out, out8, vals, pairs, "edges")
    for a, b in ((1, 129), (63, 191), (64, 192), (65, 5000), (0, m - 1), (130, 257), (4999, 5130)):
        for place in C.rmq_min_places(a, b):
            v2 = vals.copy(); v2[place] = 7                     # the range's only minimum
            out, out8 = K.rmq_query(v2, [(a, b)])
            C.check_rmq(out, out8, v2, [(a, b)], "minimum at %d of [%d, %d]" % (place, a, b))
            assert int(out[0]) == 7
    full = np.full(300, 0xFFFFFFFF, U32)
    pairs = [(0, 299), (0, 127), (1, 129), (64, 191), (5, 5)]
    out, out8 = K.rmq_query(full, pairs)
    C.check_rmq(out, out8, full, pairs, "all 0xffffffff")


# ---- one chain, tied to the product -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wp", ((10, 100), (4, 11)))
def test_chain_in_product_order(wp):
    """a small pangenome through every stage in the order of pfp.cpp: each stage gets the model's inputs and must return the
    model's outputs; at the end the model's .dict and parse are what Engine.parse_only gives for the same documents"""
    import mumemto_amd
    import pyoracle as O
    from mumemto_amd import synth
    w, p = wp
    docs = synth.pangenome(3, 3000, 0.01, seed=31, n_run=(1, 700, 790))
    text, _ = O.build_text(docs, True)
    M = P.Model(text, w, p)
    n, m, D, nd = M.n, M.m, M.D, M.dict_len
    for layout in ("bytes", "packed"):
        tx = K.Text(text, layout)
        masks, counts = K.trigger_masks(tx, w, p)
        C.check_trigger_masks(masks, counts, n, w, M.cuts, "chain " + layout)
    off = np.cumsum(M.block_count.astype(np.int64)) - M.block_count
    C.check_cuts(K.trigger_cuts(M.masks, n, off, m - 1 + 2, False), M.masks, n, "chain")
    start, length = K.phrase_bounds(M.cuts, n, w, False)
    C.column(start, K.u32(M.pstart), "pstart"); C.column(length, K.u32(M.plen), "plen")
    tx = K.Text(text)
    h1, pinfo = K.phrase_hash(tx, M.pstart, M.plen)
    C.check_phrase_hash(h1, pinfo, tx.v, M.pstart, M.plen, "chain")
    C.column(K.iota(m), np.arange(m, dtype=U32), "iota")
    C.column(K.gather_u64(M.h1, M.order), M.h1s, "h1 in order")
    C.column(K.second_fingerprint(M.pinfo), P.second_fingerprint(M.pinfo), "h2")
    flags, err = K.mark_distinct(M.order, M.h1s, M.pinfo, tx)
    C.check_mark_distinct(flags, err, tx.v, M.order, M.h1s, M.pinfo, "chain")
    assert int(err[0]) == 0 and int(err[1]) == 0
    pid, rep, dlen = K.assign_distinct(M.order, M.scan, M.dflags, M.plen, D + 2)
    C.same(pid, M.pid, "pid"); C.column(rep, M.rep, "rep"); C.column(dlen, M.dlen, "dlen")
    assert K.sum_u32(M.dlen) + 1 == nd
    for pack_prev, info_want in ((True, M.dinfo_packed), (False, M.dinfo_plain)):
        d, info = K.copy_dict(tx, M.pstart, M.plen, M.rep, M.dstart, nd, pack_prev)
        C.check_copy_dict(d, info, tx.v, M.pstart, M.plen, M.rep, M.dstart, nd, pack_prev, None, "chain pack %d" % pack_prev)
        esuf, ephr, ebw = K.entry_info(M.sa_d, info_want, M.dict, pack_prev)
        C.column(esuf, M.esuf, "esuf"); C.column(ephr, M.ephr, "ephr"); C.column(ebw, M.ebw, "ebw")
    n_long = len(M.longs)
    plcp, longs, count = K.dict_irreducible(M.dict, M.sa_d, M.esuf, M.ebw, n_long + 4, n_long + 6)
    C.check_dict_irreducible(plcp, longs, count, n_long + 4, M.dict, M.sa_d, M.esuf, M.ebw, "chain")
    C.same(K.long_lcp_lim(M.dict, sorted(M.longs), M.plcp_first), M.plcp_irr, "long_lcp_lim")
    C.column(K.plcp_running_max(M.plcp_irr), M.plcp, "PLCP")
    C.column(K.lcp_gather(M.plcp, M.sa_d), M.lcp_gathered, "gathered")
    C.check_dict_lcp(K.dict_lcp_clamp(M.lcp_gathered, M.esuf), M.dict, M.sa_d, M.esuf, "chain")
    g, pf, v, seg = K.group_flags(M.esuf, M.lcp_d, w)
    C.check_group_flags(g, pf, v, seg, M.esuf, M.lcp_d, w, "chain")
    C.same(K.scan(1, M.seg, U64), M.segmin, "segmented minimum")
    C.column(K.phrase_ranks(M.esuf, M.ephr, M.pscan, D + 2), M.prank, "prank")
    C.column(K.parse_ranks(M.pid, M.prank), M.parse, "parse")
    which, slen = K.invert_ranks(M.prank, M.rep, M.dlen)
    C.column(which, M.which, "which"); C.column(slen, M.slen, "slen")
    sl, bmin, nb, levels, n_irr, n_lg = K.parse_lcp(tx, M.nv, M.sa_p, M.pid, M.pstart, False)
    C.check_parse_lcp(sl, bmin, nb, levels, n_irr, n_lg, M, "chain")
    keys, vals = K.occ_sequence(M.sa_p, M.pid, D)
    C.check_occ_sequence(keys, vals, M.sa_p, M.pid, D, "chain")
    for mode in (8, 12):
        occ_start, occ, occ_sl = K.occ_finish(mode, M.occ_ids, M.occ_ts, M.sa_p, M.pstart, False, M.sl, M.pos_bits, D + 2)
        C.check_occ_finish(mode, occ_start, occ, occ_sl, M.occ_ids, M.occ_ts, M.sa_p, M.pstart, M.sl, M.pos_bits, "chain mode %d" % mode)
    tab = K.phrase_table(M.occ_start, M.plen, M.rep)
    C.same(tab[:D], M.tab, "tab")
    ce = K.entry_compact(M.esuf, M.ephr, M.ebw, M.gflag, M.gscan, M.vflag, M.vscan, M.segmin, M.tab, M.E)
    for k in ce:
        C.column(ce[k], M.ce[k], "ce_" + k)
    assert int(M.ce["cnt"].astype(np.int64).sum()) == n + 1    # the expansion covers the stream exactly once
    C.column(K.gather_pos(M.ce_eoff, M.sege, False), M.segb[:M.G], "segb")
    gh = K.group_heads(M.sege, M.ce["hl"], M.ce["slen"])
    C.same(gh[:M.G], M.ghead, "ghead")
    osize, err = K.oversize(M.segb, False)
    C.check_oversize(osize, err, M.segb, "chain")
    tile = K.emit_tile()
    tiles = (n + 1 + tile - 1) // tile
    C.column(K.tile_first(M.segb[:M.G], tiles, False), P.tile_first(M.segb[:M.G], tiles, tile), "tile_first")
    # the product, for the same documents
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_docs(docs)
        d, q = eng.parse_only(True, w, p)
    finally:
        eng.close()
    assert d == M.dict_file()
    C.same(q, M.parse, "parse of the product")


if __name__ == "__main__" and sys.argv[1:] == ["plain"]:
    assert os.environ.get("MMT_TRIGGER_PLAIN") == "1"
    for _w in (4, 10, 16):
        _trigger_window(_w, True)
    print("plain triggers ok")
