"""No GPU: tests/pfpmodel.py (the reference of tests/test_gpu_pfp_kernels.py) against independent statements -- the real
reference parser's files (tests/golden/newscan), a rolling Karp-Rabin, the oracle's restatement of the parse, naive suffix and
LCP computations --, the packer of tests/kprobe.py against a byte-wise reader of the layout of csrc/textref.hpp, the cases of
tests/pfp_cases.py against the boundaries they claim, and six wrong device outputs through the GPU tests' own assertion
functions: each must be rejected."""
import os

import numpy as np
import pytest

import kprobe as K
import pfp_cases as C
import pfpmodel as P
import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "newscan")
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64


def fixture(case):
    docs, cur = [], []
    for line in open(os.path.join(G, case, "input.txt"), "rb").read().split(b"\n"):
        if line.startswith(b"F $"):
            if cur:
                docs.append(cur)
                cur = []
        elif line.startswith(b"F "):
            cur.append(line[2:])
    w, p = map(int, open(os.path.join(G, case, "params.txt")).read().split())
    return O.build_text(docs, True)[0], w, p


@pytest.fixture(scope="module")
def models():
    return {case: P.Model(*fixture(case)) for case in sorted(os.listdir(G))}


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_writes_the_reference_parsers_files(models):
    for case, M in models.items():
        assert M.dict_file() == open(os.path.join(G, case, "out.dict"), "rb").read(), case
        assert M.parse.tobytes() == open(os.path.join(G, case, "out.parse"), "rb").read(), case
        assert M.err0 == 0 and M.err1 == 0


def rolling_cuts(text, w, p):
    """newscan.hpp:106-114 as tests/test_gpu_pfp.py restates it: a rolling window, never reset"""
    prime = 1999999973
    h, cuts, win, pot = 0, [], [0] * w, pow(256, w - 1, prime)
    for i, c in enumerate(bytes(text)):
        h = (h + prime - (win[i % w] * pot) % prime) % prime
        h = (h * 256 + c) % prime
        win[i % w] = c
        if h % p == 0 and i + 1 >= w:
            cuts.append(i)
    return cuts


@pytest.mark.parametrize("w", (1, 2, 4, 7, 10, 16, 31, 32))
def test_triggers_equal_the_rolling_window(w):
    for n in (1, w - 1, w, w + 1, 300, 4097):
        if n < 1:
            continue
        for name, text in C.trigger_texts(n, w).items():
            for p in C.TRIGGER_MODULI:
                assert P.triggers(text, w, p).tolist() == rolling_cuts(text, w, p), (w, n, name, p)


def test_phrases_and_dictionary_equal_a_set_of_slices(models):
    """phrases as slices of V, the dictionary as the sorted set of them, the parse as ranks (the restatement of
    tests/test_gpu_pfp.py)"""
    for M in models.values():
        v = M.v.tobytes()
        cuts = rolling_cuts(M.text, M.w, M.p)
        starts = [0] + [c - M.w + 2 for c in cuts]
        ends = [c + 1 for c in cuts] + [M.n + M.w]
        phrases = [v[a:b + 1] for a, b in zip(starts, ends)]
        assert M.pstart == starts and M.plen == [len(x) for x in phrases]
        uniq = sorted(set(phrases))
        assert M.dict_file() == b"".join(x + b"\x01" for x in uniq) + b"\x00"
        rank = {x: i + 1 for i, x in enumerate(uniq)}
        assert M.parse.tolist() == [rank[x] for x in phrases]
        assert [phrases[r] for r in M.rep] == [phrases[M.order[k]] for k in np.flatnonzero(M.dflags)]
        assert M.D == len(uniq) and M.dict_len == sum(len(x) + 1 for x in uniq) + 1


def test_statistics_equal_the_oracles_parse(models):
    for M in models.values():
        stats = O.build_stream_pfp(M.text, M.w, M.p)[3]
        assert (M.m, M.D, M.dict_len, M.n + 1) == stats
        assert int(M.ce["cnt"].astype(np.int64).sum()) == M.n + 1          # every text suffix and the sentinel, once


def test_fingerprint_fields():
    h1, rec = P.fingerprint(b"ACGT", (0xAB << 32) | 5)
    assert rec[3] == 4 and rec[2] == 5 and rec[1] >> 24 == 0xAB
    x = 0
    for c in b"ACGT":
        x = (x * P.B1 + c + 1) % (1 << 64)
    assert h1 == x ^ ((4 * P.LEN_MIX) % (1 << 64))
    assert int(P.second_fingerprint(K.u32([rec]))[0]) == ((rec[1] & 0xFFFFFF) << 32) | rec[0]
    assert P.record_start(rec) == (0xAB << 32) | 5


def naive_terminated_order(d):
    """suffixes of the dictionary as tuples that end at the first terminator, which carries its position"""
    d = [int(x) for x in d]

    def key(i):
        out = []
        for j in range(i, len(d)):
            if d[j] <= 1:
                out.append((0, j))
                break
            out.append((d[j], 0))
        return out
    return sorted(range(len(d)), key=key)


def test_dictionary_tables_against_naive_computations(models):
    M = models["tiny"]
    assert M.sa_d.tolist() == naive_terminated_order(M.dict)
    for M in models.values():
        nd = M.dict_len
        assert sorted(M.sa_d.tolist()) == list(range(nd))
        # the chain irreducible -> PLCP -> gather -> clamp gives the LCP of adjacent suffixes
        C.same(M.lcp_d, P.naive_dict_lcp(M.dict, M.sa_d, M.esuf), "lcp_d")
        # both record forms say the same
        for a, b in zip(P.entry_info(M.sa_d, M.dict, M.dinfo_packed, True), (M.esuf, M.ephr, M.ebw)):
            C.same(a, b, "entry_info, packed form")
        # suffix words: the distance to the phrase's terminator
        pos = M.sa_d.astype(np.int64)
        ends = np.flatnonzero(M.dict <= 1)
        nxt = ends[np.searchsorted(ends, pos)]
        C.same(M.esuf & U32(0x7FFFFFFF), (nxt - pos).astype(U32), "suffix lengths")
        # the parse's suffix array and sl, naively
        assert M.sa_p.tolist() == K.naive_suffix_array(M.parse).tolist() or M.m > 2000
        phr = [M.v[a:a + l].tobytes() for a, l in zip(M.pstart, M.plen)]
        assert all(phr[M.rep[M.pid[q]]] == phr[q] for q in range(M.m))
        # groups: equal valid suffixes, and only they, share a group
        valid = np.flatnonzero(M.vflag)
        sufs = [M.dict[M.sa_d[r]:M.sa_d[r] + (int(M.esuf[r]) & 0x7FFFFFFF)].tobytes() for r in valid]
        want = [1] + [int(sufs[i] != sufs[i - 1]) for i in range(1, len(sufs))]
        assert M.gflag[valid].tolist() == want
        # ghead: the LCP of the strings of adjacent groups
        firsts = [i for i in range(len(sufs)) if want[i]]
        for g in range(1, min(len(firsts), 400)):
            a, b = sufs[firsts[g] - 1], sufs[firsts[g]]
            k = 0
            while k < min(len(a), len(b)) and a[k] == b[k]:
                k += 1
            assert tuple(M.ghead[g]) == (len(b), k), g


def test_stream_order_from_the_tables():
    """the tables spell the suffix array of the text: groups in order, inside a group the occurrences by the rank t of the parse
    suffix that follows; and sl through the range minimum gives the LCP inside a group (pfp_lcp_mum.hpp:295-321)"""
    text, w, p = fixture("three_docs_w4_p11")
    text = text[:3000]
    M = P.Model(text, w, p)
    sa, lcp, _ = O.build_stream(text)
    got_sa, got_lcp = [], []
    for g in range(M.G):
        e0, e1 = int(M.sege[g]), int(M.sege[g + 1]) if g + 1 < M.G else M.E
        items = []
        for e in range(e0, e1):
            for k in range(int(M.ce["cnt"][e])):
                rec = int(M.occ[int(M.ce["first"][e]) + k])
                items.append((rec >> M.pos_bits, (rec & ((1 << M.pos_bits) - 1)) + int(M.ce["offm1"][e])))
        items.sort()
        for i, (t, pos) in enumerate(items):
            got_sa.append(pos)
            if i == 0:
                got_lcp.append(int(M.ghead[g][1]))
            else:
                got_lcp.append(int(M.ghead[g][0]) - w + int(M.sl[items[i - 1][0]:t].min()))
    assert got_sa == [int(x) for x in sa]
    assert got_lcp[1:] == [int(x) for x in lcp[1:]]


# ---- the packer ---------------------------------------------------------------------------------------------------------------------------
def unpack_byte(words, excw, runs, n, p):
    """text position p of a packed text, written from the layout at the top of textref.hpp"""
    c = (int(words[p >> 5]) >> (2 * (p & 31))) & 3
    b = p >> 12
    if (int(excw[b >> 6]) >> (b & 63)) & 1:
        for lo, hi, ln, byte in runs.tolist():
            s = lo | (hi << 32)
            if s <= p < s + ln:
                return byte
    return b"ACGT"[c]


def test_packer_round_trip():
    for n in (1, 31, 32, 33, 4095, 4096, 4097, 9000):
        for name, text in C.trigger_texts(n, 10).items():
            words, excw, runs = K.pack_text(text)
            assert len(words) == (n + 31) // 32 + 2 and int(words[-1]) == 0 and int(words[-2]) == 0
            assert bytes(unpack_byte(words, excw, runs, n, p) for p in range(n)) == text.tobytes(), (n, name)
            s = [(lo | (hi << 32), ln, b) for lo, hi, ln, b in runs.tolist()]
            assert all(s[i][0] + s[i][1] <= s[i + 1][0] for i in range(len(s) - 1))           # sorted, disjoint
            assert all(b not in b"ACGT" and ln > 0 for _, ln, b in s)
            blocks = {q >> 12 for a, ln, _ in s for q in range(a, a + ln)}
            assert {b for b in range((n >> 12) + 1) if (int(excw[b >> 6]) >> (b & 63)) & 1} == blocks
            assert runs.dtype == U32 and runs.shape[1:] == (4,)                               # the 16-byte record of ExcRun
    t = K.Text(C.rnd_text(100, 1))
    assert t.v[0] == 2 and bytes(t.v[101:133]) == b"\x02" * 32 and not t.v[133:].any() and len(t.v) >= 100 + 33 + 64


# ---- the cases hit what they claim -----------------------------------------------------------------------------------------------------------
def test_cases_reach_their_boundaries():
    for name, (text, start, lens) in C.hash_cases().items():
        assert all(b == a + l - C.HASH_W for a, l, b in zip(start, lens, start[1:])) and start[-1] + lens[-1] <= len(text) + 1
    assert max(C.hash_cases()["long2048"][2]) == 2048 == P.HASH_LONG and max(C.hash_cases()["long2049"][2]) == 2049
    (text, start, lens), idx = C.route_case()
    v = P.make_v(text)
    assert len({v[start[i]:start[i] + lens[i]].tobytes() for i in idx}) == 1 and [i // 64 for i in idx] == [0, 1, 2]
    cases = C.distinct_cases()
    text, order, h1s, pinfo = cases["runs"]
    flags, e0, e1 = P.mark_distinct(order, h1s, pinfo, P.make_v(text))
    assert (e0, e1) == (0, 0) and int(flags.sum()) == 2 * len(C.RUNS) and len(order) == 2 * sum(C.RUNS)
    text, order, h1s, pinfo = cases["collide"]
    flags, e0, e1 = P.mark_distinct(order, h1s, pinfo, P.make_v(text))
    assert e0 == 44 and e1 == 0 and flags.all()
    text, order, h1s, pinfo = cases["h1_only"]
    flags, e0, e1 = P.mark_distinct(order, h1s, pinfo, P.make_v(text))
    assert (e0, e1) == (0, 1) and flags.all() and int(h1s[64]) == int(h1s[63])
    d, sa_d, esuf, ebw = C.lcp_dictionary()
    lcp = P.naive_dict_lcp(d, sa_d, esuf)
    assert set(C.SHARED) | {C.EXACT_LIMIT} <= set(lcp.tolist())
    first, longs, full = P.dict_irreducible(d, sa_d, esuf, ebw)
    assert len(longs) >= 3 and any(lim == C.EXACT_LIMIT == full[p] for p, q, h, lim in longs)
    C.same(P.dict_lcp_clamp(P.plcp_running_max(full)[sa_d], esuf), lcp, "the chain on the forged dictionary")
    M = P.Model(C.shared_text(), C.PARSE_W, C.PARSE_P)
    assert set(C.PARSE_SHARED) <= set(M.sl.tolist()) and M.n_long >= 2
    mods = {(int(M.pstart[M.sa_p[r]]) % 8, int(M.pstart[M.sa_p[r - 1]]) % 8) for r in range(1, M.m) if M.sl[r] >= 20}
    assert len(mods) == 64                                     # every pair of start offsets mod 8
    for m in C.PARSE_M[:4]:
        assert P.Model(C.text_of_m_phrases(m, C.PARSE_W, C.PARSE_P), C.PARSE_W, C.PARSE_P, with_lists=False).m == m
    found = set()
    for w in (4, 10):
        for n in C.trigger_lengths(w):
            for text in C.trigger_texts(n, w).values():
                for p in C.TRIGGER_MODULI:
                    h = P.kr_hashes(text, w) % p
                    found |= {"at w" for i in (w - 1,) if i < n and h[i] == 0} | {"before w" for i in range(min(w - 1, n)) if h[i] == 0}
    assert found == {"at w", "before w"}                       # hits at i + 1 = w (reported) and before (suppressed)


# ---- six wrong outputs, each rejected ---------------------------------------------------------------------------------------------------------
def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_mutation_trigger_at_the_first_full_window():
    w, p = 4, 2
    for seed in range(50):
        text = C.rnd_text(100, seed)
        cuts = P.triggers(text, w, p)
        if len(cuts) and cuts[0] == w - 1:
            break
    assert cuts[0] == w - 1
    masks, counts = P.trigger_masks(100, cuts)
    ok = (np.concatenate([masks, np.full(3, 0xA5A5, U16)]), np.concatenate([counts, np.full(3, K.SENT32, U32)]))
    C.check_trigger_masks(ok[0], ok[1], 100, w, cuts)
    m2, c2 = P.trigger_masks(100, cuts[1:])                   # "i + 1 > w"
    rejected(C.check_trigger_masks, np.concatenate([m2, ok[0][-3:]]), np.concatenate([c2, ok[1][-3:]]), 100, w, cuts)


def test_mutation_fingerprint_without_the_length():
    text, start, lens = C.hash_cases()["m65"]
    v = P.make_v(text)
    h1, pinfo = P.fingerprints(v, start, lens)
    pad = lambda a, s: np.concatenate([a, np.full((2,) + a.shape[1:], s, a.dtype)])
    C.check_phrase_hash(pad(h1, K.SENT64), pad(pinfo, K.SENT32), v, start, lens)
    bare = K.u64([P.poly(v[a:a + l], P.B1) for a, l in zip(start, lens)])
    rejected(C.check_phrase_hash, pad(bare, K.SENT64), pad(pinfo, K.SENT32), v, start, lens)


def test_mutation_distinct_marking_without_the_last_partial_chunk():
    text, order, h1s, pinfo = C.distinct_cases()["collide"]
    v = P.make_v(text)
    flags, e0, e1 = P.mark_distinct(order, h1s, pinfo, v)
    err = np.full(16, K.SENT32, U32); err[0], err[1] = e0, e1
    tail = np.full(2, K.SENT32, U32)
    C.check_mark_distinct(np.concatenate([flags, tail]), err, v, order, h1s, pinfo)
    cut = pinfo.copy()
    cut[:, 3] = cut[:, 3] // 8 * 8                              # whole 8-byte chunks only
    f2, e2, _ = P.mark_distinct(order, h1s, cut, v)
    err2 = err.copy(); err2[0] = e2
    assert e2 < e0
    rejected(C.check_mark_distinct, np.concatenate([f2, tail]), err2, v, order, h1s, pinfo)


def test_mutation_dictionary_lcp_off_by_one_at_128():
    d, sa_d, esuf, ebw = C.lcp_dictionary()
    lcp = P.naive_dict_lcp(d, sa_d, esuf)
    tail = np.full(3, K.SENT32, U32)
    C.check_dict_lcp(np.concatenate([lcp, tail]), d, sa_d, esuf)
    bad = lcp.copy()
    assert (bad == 128).any()
    bad[bad == 128] = 127
    rejected(C.check_dict_lcp, np.concatenate([bad, tail]), d, sa_d, esuf)


def sl_by_running_maximum_over_values(M):
    """the mistake parse_lcp.hpp warns about: the running maximum of lirr[q] + pstart[q] instead of the last irreducible q"""
    m = M.m
    isa = np.empty(m, np.int64); isa[M.sa_p] = np.arange(m)
    base = np.zeros(m, np.int64)
    for q in range(m):
        r = int(isa[q])
        qb = int(M.sa_p[r - 1]) if r else 0
        if r == 0 or q == 0 or qb == 0 or M.pid[q - 1] != M.pid[qb - 1]:
            base[q] = int(M.sl[r]) + M.pstart[q]
    value = np.maximum.accumulate(base) - np.asarray(M.pstart, dtype=np.int64)
    out = value[M.sa_p].astype(U32)
    out[0] = 0
    return out


def test_mutation_sl_by_a_running_maximum_over_values():
    hit = 0
    for text in (C.shared_text(), C.identical_haplotypes(), C.text_of_m_phrases(4097, C.PARSE_W, C.PARSE_P)):
        M = P.Model(text, C.PARSE_W, C.PARSE_P)
        pad = np.full(8, K.SENT32, U32)
        C.check_parse_lcp(M.sl, np.concatenate([M.bmin, pad]), M.nb, M.levels, M.n_irreducible, M.n_long, M)
        bad = sl_by_running_maximum_over_values(M)
        if not np.array_equal(bad, M.sl):
            hit += 1
            nb, levels, bmin = P.rmq_tables(bad)
            rejected(C.check_parse_lcp, bad, np.concatenate([bmin, pad]), nb, levels, M.n_irreducible, M.n_long, M)
    assert hit                                                  # the cases hold a parse on which the two differ


def test_mutation_rmq_without_the_tail_stretch():
    m = 10000
    pairs = C.rmq_pairs_edges(m)
    vals = np.random.default_rng(9).integers(1000, 1 << 32, m, dtype=np.int64).astype(U32)
    want = P.rmq_answers(vals, pairs)
    C.check_rmq(want, want, vals, pairs)
    bad = K.u32([vals[a:(((b + 1) >> 6) << 6 if b - a >= P.RMQ_SCAN else b + 1)].min() for a, b in pairs])
    assert not np.array_equal(bad, want)
    rejected(C.check_rmq, bad, want, vals, pairs)
    rejected(C.check_rmq, want, bad, vals, pairs)
    # and with the only minimum in the tail stretch
    a, b = 65, 5000
    v2 = vals.copy(); v2[b] = 7
    assert int(v2[a:((b + 1) >> 6) << 6].min()) != 7 and b in C.rmq_min_places(a, b)
