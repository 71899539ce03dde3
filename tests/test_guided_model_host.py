"""CPU checks of tests/guidedmodel.py and tests/guided_cases.py: a broken model, a case generator that does not build what it
claims, or a designed case that the probe library would reject must fail here, without a GPU -- not let
tests/test_gpu_guided_kernels.py pass vacuously.  Also the census: every wrapper declared in csrc/guided_kernels.hpp has a
probe and a model function, or stands in the list of those that have none, with its reason."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import guided_cases as C      # noqa: E402
import guidedmodel as GM      # noqa: E402
import kprobe as K            # noqa: E402

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
ROOT = os.path.dirname(HERE)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def declared_wrappers():
    return re.findall(r"^void\s+(\w+)\(", _read("mumemto_amd", "csrc", "guided_kernels.hpp"), re.M)


def test_every_wrapper_has_a_probe_or_a_reason():
    names = declared_wrappers()
    assert len(names) == len(set(names)) and len(names) >= 45, names
    probe_src = _read("tests", "kprobe", "kprobe.cpp")
    gpu_test = _read("tests", "test_gpu_guided_kernels.py")
    header = gpu_test[:gpu_test.index('"""', 3)]
    tested = set(re.findall(r"^def test_(\w+?)(?:__\w+)?\(", gpu_test, re.M))
    covered = []
    for name in names:
        has = [hasattr(K, "gk_" + name), hasattr(GM, name), ("KP int kp_gk_%s(" % name) in probe_src]
        if name in C.NOT_COVERED:
            assert not any(has), "%s is listed as not covered but has a probe or a model" % name
            assert C.NOT_COVERED[name].strip()
            assert re.search(r"\b%s\b" % name, header), "%s missing from the header of test_gpu_guided_kernels.py" % name
        else:
            assert all(has), "%s: wrapper without probe (kprobe.cpp, kprobe.py) and model (guidedmodel.py): %s" % (name, has)
            assert name in tested, "%s has a probe but no test_%s in test_gpu_guided_kernels.py" % (name, name)
            covered.append(name)
    assert set(C.NOT_COVERED) <= set(names), "a name in NOT_COVERED is not a wrapper"
    assert len(covered) + len(C.NOT_COVERED) == len(names)


def test_mirrored_precondition_messages_are_the_probe_library_s():
    src = _read("tests", "kprobe", "kprobe.cpp")
    mirror = _read("tests", "guided_cases.py")
    msgs = re.findall(r'return "([^"]+)"', mirror[mirror.index("mirrored"):])
    assert len(msgs) >= 12
    for m in msgs:
        assert '"%s"' % m in src, m


# ---- phrase ends -------------------------------------------------------------------------------------------------------------
def test_cut_cases_hold_what_they_claim():
    cases = C.cut_cases()
    assert len(cases) == 13
    assert sorted({n for n, _ in cases.values()}) == [1, 4095, 4096, 4097, 3 * 4096 + 5, C.MAX_TEXT]
    for name, (n, cuts) in cases.items():
        assert n <= C.MAX_TEXT and cuts == sorted(set(cuts)) and all(0 <= c < n for c in cuts), name
    for name, want in C.CUT_BLOCK_COUNTS.items():
        n, cuts = cases[name]
        got = np.bincount(np.array(cuts) // 4096, minlength=len(want)).tolist()
        assert got == want, (name, got)
    n, cuts = cases["gap_then_zero"]
    per = np.bincount(np.array(cuts) // 4096, minlength=3)
    assert per[1] == 0 and 2 * 4096 in cuts
    n, cuts = cases["edges_%d" % (3 * 4096 + 5)]
    assert cuts == [0, 63, 64, 511, 512, 4095, 4096, n - 1]


def test_cut_tables_against_naive_counts():
    for name, (n, cuts) in C.cut_cases().items():
        t = GM.CutTables(cuts, n, 5)
        c = np.array(cuts, dtype=np.int64)
        assert GM.cuts_of_mask(t.mask) == cuts and t.n_blocks >= n // 4096 + 2, name
        assert t.rdir.tolist() == [int((c < 512 * j).sum()) for j in range(len(t.rdir))], name
        assert t.brank.tolist() == [int((c < 4096 * b).sum()) for b in range(t.n_blocks + 2)], name
        assert t.coff[:len(cuts)].tolist() == [x & 4095 for x in cuts], name
        for b in range(t.n_blocks + 1):
            later = [x for x in cuts if x >= 4096 * b]
            assert int(t.nxt[b]) == (later[0] if later else n + 5 - 1), (name, b)


def test_phrase_end_layouts_agree():
    """rdir / mask and coff / brank answer every next_cut / rank1 query as the definition does"""
    queries = 0
    for name, (n, cuts) in C.cut_cases().items():
        for w in (4, 10):
            t = GM.CutTables(cuts, n, w)
            for x in range(n + w + 3):
                nc, r = t.next_cut(x), t.rank1(x)
                if x % 97 == 0 or x < 70 or x >= n - 2:                  # the definition itself, by a plain scan
                    assert nc == (min([c for c in cuts if c >= x], default=n + w - 1) if x < n else n + w - 1), (name, x)
                    assert r == sum(1 for c in cuts if c < x), (name, x)
                assert t.next_cut_bits(x) == nc and t.next_cut_list(x) == nc, (name, x)
                assert t.rank1_bits(x) == r and t.rank1_list(x) == r, (name, x)
                queries += 1
    assert queries > 150000


# ---- first keys and rounds ---------------------------------------------------------------------------------------------------
def test_heads0_model_against_bit_strings():
    cases = C.heads0_cases()
    assert len(cases) == 2 * (8 + 1)
    seen_first = seen_last = False
    for name, (keys, bits, chars) in cases.items():
        B = len(keys)
        assert np.all(keys[1:] >= keys[:-1]), name
        head, active, lcp = GM.heads0(keys, bits, chars, np.zeros(B, U8), np.zeros(B, U8), np.full(B, 0xFFFFFFFF, U32))
        strings = [format(int(k), "0%db" % (bits * chars)) for k in keys]
        for j in range(B):
            size = strings.count(strings[j])
            assert head[j] == (1 if j == 0 or strings[j] != strings[j - 1] else 0)
            assert active[j] == (1 if size > 1 else 0)
            if j and head[j]:
                common = next(i for i in range(bits * chars) if strings[j][i] != strings[j - 1][i])
                assert lcp[j] == common // bits
                seen_first |= lcp[j] == 0
                seen_last |= lcp[j] == chars - 1
            else:
                assert lcp[j] == 0xFFFFFFFF
        if name.startswith("chain"):
            assert sorted(int(x) for x in lcp if x != 0xFFFFFFFF) == list(range(chars)), name
            assert int(keys[-1]) >> (bits * chars - 1) == 1                 # the top bit of the key: bit 62 when 63 bits
    assert seen_first and seen_last
    assert {len(k) for k, _, _ in cases.values()} >= {1, 2, 256, 257}


def test_medium_cases_and_model():
    cases = C.medium_cases()
    for name, (sizes, cap) in cases.items():
        gh = C.gheads(sizes)
        assert GM.groups_of(gh) == list(zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist(), sizes)), name
        regions, counts = GM.medium_groups(gh)
        for cl, (lo, hi) in enumerate(((1, 16), (17, 32), (33, 64), (65, 128))):
            assert sorted(s for _, s in regions[cl]) == sorted(s for s in sizes if lo <= s <= hi), name
        assert all(s != 129 and s != 130 for r in regions for _, s in r)
        assert max(counts) <= cap, name
    assert set(cases["each_size"][0]) == {1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129}
    sizes, cap = cases["many_exact_cap"]
    assert sum(sizes) > 3 * 1024 and max(GM.medium_groups(C.gheads(sizes))[1]) == cap
    assert cases["ends_with_129"][0][-1] == 129 and cases["ends_with_9"][0][-1] == 9


def test_tile_bounds_model_against_the_sorter_s_reference():
    """kprobe.ref_bounds (the suffix sorter's round_head_bounds, written and checked on its own) states the same rule"""
    seen = set()
    for name, (sizes, target, limit, n_tiles) in C.bounds_cases().items():
        gh = C.gheads(sizes)
        got = GM.tile_bounds(gh, target, limit, n_tiles, np.zeros(n_tiles + 1, U32))
        assert np.array_equal(got, K.ref_bounds(gh, target, limit, n_tiles)), name
        m = len(gh)
        for t in range(1, n_tiles):
            b = int(got[t])
            seen.add("none" if b == GM.NO_BOUND else ("m" if b == m else ("exact" if b == t * target else "later")))
        if m % target:
            seen.add("ragged")
    assert seen == {"none", "m", "exact", "later", "ragged"}
    c = C.bounds_cases()
    assert int(GM.tile_bounds(C.gheads(c["limit_one_short"][0]), 8, 8, 3, np.zeros(4, U32))[1]) == GM.NO_BOUND
    assert int(GM.tile_bounds(C.gheads(c["limit_just_reaches"][0]), 8, 9, 3, np.zeros(4, U32))[1]) == 16


def test_sort_cases_and_local_sort_model():
    lens, networks, counted = set(), 0, 0
    for sc in C.sort_cases():
        assert C.reject_local_sort(sc.ghead, sc.bound, 0, 0) is None, sc.name
        ranges = GM.tile_ranges(sc.bound)
        assert sum(e - b for b, e in ranges) == sc.m and len(set(sc.pin.tolist())) == sc.m, sc.name
        lens |= {e - b for b, e in ranges}
        kout, pout, big, network = GM.local_sort(sc.kin, sc.pin, sc.ghead, sc.bound, np.full(sc.m, K.SENT64, U64),
                                                 np.full(sc.m, K.SENT64, U64), 4)
        assert len(big) == sc.n_big
        networks += len(network)
        for b, e in ranges:
            if (b, e) in big:
                assert e - b > GM.SORT_CAP and np.all(kout[b:e] == U64(K.SENT64)) and np.all(pout[b:e] == U64(K.SENT64))
                continue
            counted += (b, e) not in network
            where = {int(p): i for i, p in enumerate(sc.pin)}
            src = [where[int(p)] for p in pout[b:e]]
            assert sorted(src) == list(range(b, e))                              # a permutation of the tile
            assert np.array_equal(kout[b:e], sc.kin[src])
            trip = [(int(sc.ghead[i]), int(sc.kin[i]), i) for i in src]
            assert trip == sorted(trip)                                          # by (group, key), stable
            longest = max(np.bincount(sc.ghead[b:e] - U32(b)))
            assert ((b, e) in network) == (longest > GM.SHORT)
        if sc.name == "equal_keys":
            assert len(set(sc.kin.tolist())) <= 2
    assert {1, 2047, 2048, 2049} <= lens
    assert networks >= 4 and counted >= 6                                        # at least one bitonic tile (and the count path)
    sizes = [s for sc in C.sort_cases() for s in sc.sizes]
    assert 64 in sizes and 65 in sizes
    assert any(GM.NO_BOUND in sc.bound[-3:].tolist() for sc in C.sort_cases())  # tiles that begin inside the last group
    assert any(len(GM.tile_ranges(sc.bound)) < sum(1 for b in sc.bound[:-1] if b != GM.NO_BOUND) for sc in C.sort_cases())   # an empty tile


def test_range_cases_and_model():
    for name, (sizes, ranges) in C.range_cases().items():
        gh = C.gheads(sizes)
        begins, ends = [b for b, _ in ranges], [e for _, e in ranges]
        assert C.reject_range_groups(gh, begins, ends, len(gh)) is None, name
        got = GM.range_groups(gh, begins, ends)
        heads = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        want = []
        for b, e in ranges:
            for h0, h1 in zip(heads[:-1], heads[1:]):
                if b < h1 <= e:
                    want.append((h0, h1))                       # a group that ends inside the range
                elif h0 < e < h1 and e > b:
                    want.append((h0, e))                        # the group the range's end cuts
        assert got == sorted(want), name
    assert len(GM.range_groups(C.gheads([10, 10, 10]), [0, 20], [15, 30])) == 3


def test_round_apply_and_compact_models():
    newhead = np.array([0, 1, 1, 3, 4, 4, 4, 7], U32)
    slot = np.array([10, 11, 12, 13, 14, 15, 16, 17], U32)
    pos = np.arange(100, 108, dtype=U64)
    out, flags = GM.round_apply(pos, newhead, slot, np.full(20, 9, U64), np.full(9, 5, U8))
    assert flags.tolist() == [0, 1, 1, 0, 1, 1, 1, 0, 5]
    assert [i for i in range(20) if out[i] != 9] == [10, 13, 17] and out[13] == 103
    so, po, ho = GM.round_compact([1, 2, 4, 5, 6], slot, pos, newhead, np.zeros(6, U32), np.zeros(6, U64), np.full(6, 77, U32))
    assert so.tolist() == [11, 12, 14, 15, 16, 0] and po.tolist()[:5] == [101, 102, 104, 105, 106]
    assert ho.tolist() == [0, 0, 2, 0, 0, 77]                   # heads carry their NEW index, the others 0 (a running maximum follows)


def test_bookkeeping_models():
    assert GM.flag_spread(np.array([0, 0, 1, 0, 0, 0, 1], U32), np.zeros(8, U32)).tolist() == [0, 1, 1, 1, 0, 1, 1, 0]
    assert GM.giant_bits(np.array([1] + [0] * 31 + [5], U32), np.full(3, 9, U32)).tolist() == [1, 1, 9]
    assert GM.giant_bits(np.array([0] * 31 + [2], U32), np.full(2, 9, U32)).tolist() == [0x80000000, 9]
    assert GM.rep_bits(np.array([0, 1, 0, 2], U32), np.array([0, 1, 3], U32), np.zeros(1, U32)).tolist() == [0b1011]
    assert GM.add_offset(np.array([0xFFFFFFFF, 1, 7], U32), 2, 3).tolist() == [2, 4, 7]
    assert GM.add_offset(np.array([0xFFFFFFFF, 1], U64), 2, 1 << 33).tolist() == [0xFFFFFFFF + (1 << 33), 1 + (1 << 33)]
    assert GM.giant_group_flags(np.array([5, 5 | 1 << 31, 5, 4], U32), np.array([0, 5, 4, 9], U32), np.zeros(4, U32)).tolist() == [1, 0, 1, 1]
    assert GM.group_ids(np.array([1, 0, 1, 7], U32), np.array([1, 1, 2, 9], U32), 3).tolist() == [1, 0, 2, 7]
    assert GM.stage_count(np.array([(3 << 12) | 5, (4 << 12), (9 << 12) | 4095], U32), 4, 10, np.zeros(1, U32)).tolist() == [2]
    # tile offsets 0, 0, 5000, 5000, 9000 of a list of 9001 entries: entry 0 lies in tile 1 (tile 0 is empty), 4096 in tile 1,
    # 8192 in tile 3 (tile 2 is empty); the entry behind the last block names the last tile
    assert GM.stage_block_tiles(np.array([0, 0, 5000, 5000, 9000], U32), 5, 9001, np.full(5, 99, U32)).tolist() == [1, 1, 3, 4, 99]


# ---- the context ---------------------------------------------------------------------------------------------------------------
def test_text_cases_hold_what_they_claim():
    texts = C.text_cases()
    assert {len(t) for t in texts.values()} >= {4095, 4096, 4097, 3 * 4096 - 1, 3 * 4096, 3 * 4096 + 1, 2 * 4096 + 63, 2 * 4096 + 64}
    assert max(len(t) for t in texts.values()) <= C.MAX_TEXT
    for at in (4095, 4096, 4096 + 63, 4096 + 64):
        t = texts["exception@%d" % at]
        assert [int(i) for i in np.flatnonzero(~np.isin(t, np.frombuffer(b"ACGT", U8)))] == [at]
    assert set(texts["runs"][4096:8192].tolist()) == {ord("T")} and texts["runs"][4095] != ord("T") and texts["runs"][8192] != ord("T")
    assert ord("G") not in texts["no_G"]
    code, bits, chars = C.full_code()
    assert (bits, chars) == (3, 21) and [int(code[b]) for b in b"\x02$ACGNT"] == [1, 2, 3, 4, 5, 6, 7]      # N between G and T
    # the dense tiles' condition: exactly 64 characters behind the last full tile, and one fewer
    c63, c64 = C.make_ctx(texts["plain63"]), C.make_ctx(texts["plain64"])
    assert GM.dense_tiles(c63, "packed") == [0] and GM.dense_tiles(c64, "packed") == [0, 1] and GM.dense_tiles(c64, "bytes") == []
    assert GM.dense_tiles(C.make_ctx(texts["no_G"], code=GM.code_table(texts["no_G"])), "packed") == []
    assert GM.dense_tiles(C.make_ctx(texts["exception@4096"]), "packed") == [2]
    assert GM.dense_tiles(C.make_ctx(texts["exception@4095"]), "packed") == [1, 2]
    # a launch with both kinds of tiles, and tens to hundreds of phrases a tile
    c = C.make_ctx(texts["runs"])
    d = GM.dense_tiles(c, "packed")
    assert 0 < len(d) < c.tiles and 30 <= c.m / c.tiles <= 200


def test_context_model_one_by_one_and_all_at_once():
    for name in ("n=1x4096+1", "exception@4096", "runs"):
        for kw in ({}, {"rec": "rank"}, {"rep": "alternate"}, {"skip": 1}):
            c = C.make_ctx(C.text_cases()[name], **kw)
            keys, recs, keep = c.all_suffixes()
            for p in list(range(0, c.n, 37)) + list(range(c.n - 40, c.n)):
                assert int(keys[p]) == c.pack_chars(p + 1) and int(recs[p]) == c.make_rec(p + 1), (name, kw, p)
                if not kw.get("skip"):
                    assert bool(keep[p]) == c.keep(p)
                assert int(c.bins(4)[p]) == c.bin_of(p, 4)
                q = p + 1
                alpha = c.alpha_len(q)
                assert alpha >= c.w and c.rec_len(recs[p]) == alpha and c.rec_len(q | (GM.LEN_SAT << 40) if not c.rec_rank else recs[p]) == alpha
                k = c.phrase_of(q)
                if not kw.get("skip"):                                   # a suffix lies in its phrase and ends with it
                    assert c.phrase_start(k) < q and q + alpha == c.phrase_start(k) + c.phrase_len(k)
            # bins against the text itself
            v = bytes([2]) + bytes(c.text) + bytes([2]) * 32 + bytes(64)
            hist = GM.bin_hist(c, 2, np.zeros(64, U64))
            naive = {}
            for p in range(c.n):
                if c.keep(p):
                    b = int(c.code[v[p + 1]]) * 8 + int(c.code[v[p + 2]])
                    naive[b] = naive.get(b, 0) + 1
            assert {b: int(x) for b, x in enumerate(hist) if x} == naive


def test_closed_form_run_order():
    """sorted by bucket the suffixes c^r X of the run bin are in suffix order wherever the buckets differ, and K itself
    (X0 < c ? r : 2^41 - r) orders all of them: runs of 1 .. 600, preceded and followed by symbols below and above c"""
    rng = np.random.default_rng(12)
    parts = []
    for r in list(range(1, 40)) + [255, 256, 257, 300, 511, 512, 600]:
        parts.append(bytes(rng.choice(list(b"ACT"), 3)) + b"G" * r + bytes([int(rng.choice(list(b"ACT")))]))
    text = np.frombuffer(b"".join(parts)[:C.MAX_TEXT], U8)
    c = C.make_ctx(text)
    sym = int(c.code[ord("G")])
    first, lead, follow = GM.tile_lead(c, np.zeros(c.tiles, U8), np.zeros(c.tiles, U16), np.zeros(c.tiles, U8))
    whole, fol = GM.chain_leads(first, lead, follow, c.tiles)
    rs = GM.RunSlice(sym, 0, 2 * GM.RUN_BUCKETS_HALF, whole, first, fol)
    sufs = [p for p in range(c.n) if text[p] == ord("G")]
    v = bytes(text) + bytes([2])
    order = sorted(sufs, key=lambda p: v[p:])
    ks, buckets = [], []
    for p in order:
        r = 0
        while p + r < c.n and text[p + r] == ord("G"):
            r += 1
        nxt = int(c.code[v[p + r]])
        assert GM.run_at(c, rs, p) == (r, GM.run_bucket(r, nxt < sym)), p
        ks.append(r if nxt < sym else (1 << 41) - r)
        buckets.append(GM.run_bucket(r, nxt < sym))
    assert ks == sorted(ks) and buckets == sorted(buckets) and len(set(buckets)) > 80
    assert GM.run_bucket(255, True) == 255 and GM.run_bucket(256, True) == 256 and GM.run_bucket(511, True) == 511 and GM.run_bucket(512, True) == 512
    assert GM.run_bucket(2 ** 40 - 1, True) == GM.RUN_BUCKETS_HALF - 1 == GM.run_bucket(2 ** 40 + 5, True)
    assert GM.run_bucket(1, False) == 2 * GM.RUN_BUCKETS_HALF - 2 and GM.run_bucket(2 ** 40, False) == GM.RUN_BUCKETS_HALF


def test_giant_tables_are_consistent():
    c = C.make_ctx(C.text_cases()["runs"], g_depth=42)
    c.giant = g = C.real_giant(c)
    longs = [k for k in range(c.m) if c.phrase_len(k) > 42]
    assert 0 < sum(g.flag) < len(longs) and all(c.phrase_len(int(k)) > 42 for k in g.k)
    bits = c.bitwords(g.flag)
    ranks = g.rank_words(bits)
    for j, k in enumerate(g.k):
        k = int(k)
        assert (int(bits[k >> 5]) >> (k & 31)) & 1 and int(ranks[k >> 5]) + bin(int(bits[k >> 5]) & ((1 << (k & 31)) - 1)).count("1") == j
        q = c.phrase_start(k) + 1                                            # the first suffix inside the occurrence
        assert c.phrase_of(q) == k and c.giant_entry(q, 3) == int(g.isa[int(g.base[j]) + 4])
        assert int(g.base[j]) + c.phrase_len(k) <= len(g.isa)


# ---- the whole-batch chain -----------------------------------------------------------------------------------------------------
def _chain_text(seed):
    """copies of two loci with planted substitutions, a run of N and a microsatellite, a few thousand characters"""
    rng = np.random.default_rng(seed)
    loci = [C._bases(rng, 300), C._bases(rng, 220)]
    parts = []
    for i in range(14):
        s = loci[i % 2].copy()
        for x in rng.integers(0, len(s), int(rng.integers(0, 3))):
            s[x] = b"ACGT"[int(rng.integers(0, 4))]
        parts += [s, C._bases(rng, int(rng.integers(5, 40)))]
        if i == 4:
            parts.append(np.full(150, ord("N"), U8))
        if i == 9:
            parts.append(np.frombuffer(b"ACG" * 60, U8))
    return np.concatenate(parts)


def _real_ctx(text, w, p, rec, g_depth=0):
    """a context over the REAL parse of the text (tests/pfpmodel.py triggers): isa_p and sl by naive sorts of V"""
    import pfpmodel as P
    n = len(text)
    cuts = [int(x) for x in P.triggers(text, w, p) if x < n]
    v = bytes([2]) + bytes(text) + bytes([2]) * w
    code, bits, chars = C.full_code()
    c = GM.Ctx(text, w, cuts, code, bits, chars, pos_bits=20 if rec == "rank" else 40, rec_rank=1 if rec == "rank" else 0, g_depth=g_depth)
    starts = [c.phrase_start(k) for k in range(c.m)]
    sa_p = sorted(range(c.m), key=lambda k: v[starts[k]:])
    isa = np.zeros(c.m, U32)
    isa[sa_p] = np.arange(c.m, dtype=U32)
    c.isa_p = isa
    spelled = {}
    c.pid = np.array([spelled.setdefault(v[starts[k]:starts[k] + c.phrase_len(k)], len(spelled)) for k in range(c.m)], dtype=U32)
    sl = np.zeros(c.m, U32)
    for r in range(1, c.m):
        a, b = v[starts[sa_p[r]]:], v[starts[sa_p[r - 1]]:]
        t = 0
        while t < min(len(a), len(b)) and a[t] == b[t]:
            t += 1
        sl[r] = t
    if g_depth:
        c.giant = GM.derive_giant(c)
    c._all = None
    return c, sl, v


def test_whole_batch_chain_gives_the_naive_suffix_array_bwt_and_lcp():
    """bin histogram -> batch fill -> first sort -> heads0 -> gather -> small / medium / rounds -> write_columns / batch_lcp,
    chained as guided.cpp chains the wrappers, against sorted(range(n), key = the suffix of V): the suffix array restricted to
    every batch's bins, the BWT bytes, and the LCP column -- computed with the hints the sort leaves and without them, which
    must be the same column.  Real parses (w, p), records with lengths and with ranks, with and without a giant dictionary,
    and with the group kernels switched off so that the rounds and the tail do the work."""
    totals = {}
    for seed, w, p, rec, g_depth, switches in ((1, 4, 11, "len", 0, {}), (2, 6, 23, "rank", 0, {}), (3, 5, 17, "len", 42, {}),
                                                (4, 8, 30, "rank", 21, {"small": False}), (5, 4, 7, "len", 0, {"medium": False, "tail": False}),
                                                (6, 10, 29, "len", 42, {"small": False, "tail": False})):
        text = _chain_text(seed)
        n = len(text)
        assert n <= C.MAX_TEXT
        c, sl, v = _real_ctx(text, w, p, rec, g_depth)
        assert 20 <= c.m and all(c.phrase_len(k) >= w for k in range(c.m))
        sa = sorted(range(n), key=lambda i: v[i + 1:])
        true_lcp = [0]
        for a, b in zip(sa[:-1], sa[1:]):
            x, y = v[a + 1:], v[b + 1:]
            t = 0
            while t < min(len(x), len(y)) and x[t] == y[t]:
                t += 1
            true_lcp.append(t)
        pc = 2
        nb = 1 << (c.bits * pc)
        hist = GM.bin_hist(c, pc, np.zeros(nb, U64))
        assert int(hist.sum()) == n
        edges = [0, int(c.code[ord("C")]) << c.bits, (int(c.code[ord("G")]) << c.bits) + 3, int(c.code[ord("T")]) << c.bits, nb]
        base, carry = 0, None
        got_sa, got_bwt, got_lcp = np.zeros(n, U32), np.zeros(n, U8), np.zeros(n, U32)
        for lo, hi in zip(edges[:-1], edges[1:]):
            counts = GM.batch_count(c, pc, lo, hi, np.zeros(c.tiles, U32))
            B = int(counts.sum())
            assert B == int(hist[lo:hi].sum())
            off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(U32)
            keys, pos, _ = GM.batch_fill(c, pc, lo, hi, off, np.zeros(B, U64), np.zeros(B, U64), 0, 0, None)
            stats = {}
            out, hints = GM.sort_batch(c, sl, keys, pos, hints=True, stats=stats, **switches)
            out2, none = GM.sort_batch(c, sl, keys, pos, hints=False, **switches)
            assert np.array_equal(out, out2) and none is None
            for k_, v_ in stats.items():
                totals[k_] = totals.get(k_, 0) + v_
            totals["hints"] = totals.get("hints", 0) + int((hints != 0xFFFFFFFF).sum())
            got_sa, _, got_bwt = GM.write_columns(c, out, base, got_sa, None, got_bwt)
            with_hints, err1 = GM.batch_lcp(c, sl, out, carry, hints, np.zeros(16, U32))
            without, err2 = GM.batch_lcp(c, sl, out, carry, np.full(B, 0xFFFFFFFF, U32), np.zeros(16, U32))
            assert np.array_equal(with_hints, without), (seed, lo, np.flatnonzero(with_hints != without)[:5])
            assert not err1.any() and not err2.any()
            got_lcp[base:base + B] = with_hints
            if B:
                carry = out[-1:].copy()
            base += B
        assert base == n
        assert got_sa.tolist() == sa, seed
        assert got_bwt.tolist() == [0 if i == 0 else v[i] for i in sa], seed
        assert got_lcp.tolist() == true_lcp, (seed, [j for j in range(n) if got_lcp[j] != true_lcp[j]][:5])
    for step in ("small", "medium", "rounds", "tail", "hints"):
        assert totals.get(step, 0) > 0, (step, totals)


def test_no_designed_case_is_rejected_by_the_probes_preconditions():
    """the cases of the GPU tests through the mirrored precondition checks: none is rejected (a rejection on the GPU is a loud
    ProbeError, never a skipped comparison -- this shows it before a GPU is needed)"""
    checked = 0
    for name, (n, cuts) in C.cut_cases().items():
        t = GM.CutTables(cuts, n, 5)
        assert C.reject_block_cut_offsets(t.mask, t.brank, t.n_blocks, len(cuts) + 5) is None, name
        c = GM.Ctx(C._bases(np.random.default_rng(n), n), 5, cuts, *C.full_code(), isa_p=np.arange(len(cuts) + 1, dtype=U32))
        assert C.reject_ctx(c, 1) is None, name
        checked += 2
    for name, (sizes, cap) in C.medium_cases().items():
        assert C.reject_medium_groups(C.gheads(sizes), cap, 4 * cap + 3) is None, name
        checked += 1
    for name, text in C.text_cases().items():
        for kw in ({}, {"rec": "rank"}, {"rep": "alternate"}, {"skip": 1}, {"expand": 1}):
            assert C.reject_ctx(C.make_ctx(text, **kw), None if kw.get("skip") else 4) is None, (name, kw)
            checked += 1
    for name, (muts, ends) in C.pair_cases().items():
        for rec in ("rank", "len"):
            loc = C.Locus(muts, ends, rec=rec, g_depth=42 if rec == "len" else 0)
            assert C.reject_ctx(loc.c) is None and C.reject_compared(loc.c, loc.members(30), 21) is None, name
            checked += 1
    loc = C.Locus([[]] * 10, [329] * 10, skip=1)
    assert C.reject_ctx(loc.c) is None and C.reject_compared(loc.c, loc.phrases(), 21) is None
    assert C.reject_compared(loc.c, [5 | (9000 << 40)], 0) is not None and C.reject_ctx(C.make_ctx(C.text_cases()["no_G"], skip=1), 4) is not None
    assert checked == 26 + 5 + 80 + 26
