"""Cases and assertion functions of tests/test_gpu_pfp_kernels.py: the inputs on which each kernel of the prefix-free parse can
go wrong (every boundary is named here by its value) and the checks of a device output against tests/pfpmodel.py.  No GPU is
touched here: the case builders and the checks are plain numpy, so tests/test_pfp_model_host.py runs the same checks on
mutated outputs and shows that each of them can fail.

Out of reach at these sizes, and left out on purpose: the high byte of a phrase start in phrase_hash (a text beyond 4 G
characters) and the second sizing attempt of the long list in ParseLcp::build (more than 65536 matches beyond 512
characters)."""
import numpy as np

import kprobe as K
import pfpmodel as P

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
ACGT = np.frombuffer(b"ACGT", U8)


def rnd_text(n, seed):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)]


# ---- generic checks ---------------------------------------------------------------------------------------------------------
def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = np.argwhere(got != want)[0]
        raise AssertionError("%s: first difference at %s: got %s, expected %s" % (what, tuple(i), got[tuple(i)], want[tuple(i)]))


def untouched(arr, used, what):
    """everything behind the first `used` entries still holds the caller's sentinel pattern"""
    tail = np.asarray(arr)[used:]
    assert tail.size, what + ": no sentinel entries to look at"
    assert np.all(tail.view(U8) == K.SENT8), what + ": written behind entry %d" % used


def column(got, want, what):
    """the first len(want) entries equal `want`, the rest is untouched"""
    same(np.asarray(got)[:len(want)], want, what)
    untouched(got, len(want), what)


# ---- triggers -----------------------------------------------------------------------------------------------------------------
FAST_WINDOWS = (4, 6, 8, 10, 12, 14, 16)                  # the instantiations of k_trigger_masks_fast
GENERIC_WINDOWS = (1, 2, 3, 5, 7, 31, 32)
TRIGGER_MODULI = (2, 11, 16, 100, 3 << 20, P.KR_PRIME)    # q = 1 (2, 16), small odd, mixed, a large odd part, the prime itself


def trigger_lengths(w):
    """one workgroup covers 256 x 16 = 4096 positions"""
    return sorted({1, 15, 16, 17, w - 1, w, w + 1, 4095, 4096, 4097, 8193} - {0})


def trigger_texts(n, w, seed=1):
    """random ACGT; N runs that straddle position 4096 and the end of the text, and a '$'; a run of one byte of length 3 w"""
    t = rnd_text(n, seed * 1000 + n)
    runs = t.copy()
    runs[max(0, n - 5):] = ord("N")
    if n > 4100:
        runs[4090:4101] = ord("N")
    if n > 40:
        runs[n // 2] = ord("$")
        runs[7:12] = ord("N")
    one = t.copy()
    at = min(n // 3, max(0, n - 3 * w))
    one[at:at + 3 * w] = ord("A")
    return {"random": t, "n_runs": runs, "run_3w": one}


def check_trigger_masks(masks, counts, n, w, cuts, what=""):
    """masks and per-workgroup counts against the model's trigger positions; nothing behind ceil(n / 16) masks and behind the
    workgroups' counts; no trigger at i + 1 < w"""
    want_masks, want_counts = P.trigger_masks(n, cuts)
    t = (n + 15) // 16
    column(masks, want_masks, what + " masks")
    column(counts, want_counts, what + " block_count")
    pop = np.zeros(P.trigger_blocks(n) * 256, np.int64)
    pop[:t] = [bin(int(x)).count("1") for x in np.asarray(masks)[:t]]
    same(pop.reshape(-1, 256).sum(axis=1), np.asarray(counts)[:P.trigger_blocks(n)].astype(np.int64), what + " block_count = popcount")
    for i in range(min(w - 1, n)):
        assert not (int(masks[i >> 4]) >> (i & 15)) & 1, what + ": a trigger at i + 1 < w (i = %d)" % i


def forged_masks(n, kind):
    """legal mask arrays for trigger_cuts (no bit at or behind n): all set, none, one bit in work-item 63 / 64 / 255 / 256"""
    t = (n + 15) // 16
    m = np.zeros(t, U16)
    if kind == "all":
        m[:] = 0xFFFF
        if n % 16:
            m[-1] = (1 << (n % 16)) - 1
    elif kind != "none":
        m[int(kind)] = 1 << (int(kind) % 16)
    return m


CUT_KINDS = ("all", "none", "63", "64", "255", "256")
CUT_N = 3 * 4096 + 16 * 100 + 5                            # three whole workgroups and a partial one with a partial last mask


def check_cuts(cuts, masks, n, what=""):
    column(cuts, np.asarray(P.cuts_of_masks(masks, n), dtype=cuts.dtype), what + " cuts")


# ---- phrase hash ----------------------------------------------------------------------------------------------------------------
HASH_W = 10


def chained_phrases(lens, w, seed, fixed=None, first_start=1):
    """a text and consecutive phrases (start, length) that overlap by w characters, as a parse's do; fixed: index -> content
    (the phrase before it is made to end with that content's first w characters)"""
    rng = np.random.default_rng(seed)
    fixed = fixed or {}
    prev_tail = ACGT[rng.integers(0, 4, w)]
    pieces = [ACGT[rng.integers(0, 4, first_start - 1)], prev_tail]        # phrase 0 begins at V index first_start
    start, pos = [], first_start
    for k, l in enumerate(lens):
        assert l > w
        if k in fixed:
            c = np.asarray(fixed[k], dtype=U8)
            assert len(c) == l and np.array_equal(c[:w], prev_tail)
        else:
            c = np.concatenate([prev_tail, ACGT[rng.integers(0, 4, l - w)]])
            if k + 1 in fixed:
                c[l - w:] = np.asarray(fixed[k + 1], dtype=U8)[:w]
                assert l >= 2 * w
        start.append(pos)
        pieces.append(c[w:])
        pos += l - w
        prev_tail = c[l - w:]
    return np.concatenate(pieces), start, list(lens)


def hash_cases():
    """name -> (text, start, len).  m = 1, 63, 64, 65, 128, 300; a wave with a phrase of 2048 and one of 2049 characters (the
    whole-wave route begins behind 2048); a wave whose span from the aligned-down start is HASH_SPAN = 4096 bytes, and 4097"""
    out = {}
    rng = np.random.default_rng(5)
    for m in (1, 63, 64, 65, 128, 300):
        out["m%d" % m] = chained_phrases(rng.integers(HASH_W + 1, 41, m).tolist(), HASH_W, 100 + m)
    for big in (2048, 2049):
        lens = rng.integers(HASH_W + 1, 41, 130).tolist()
        lens[70] = big
        out["long%d" % big] = chained_phrases(lens, HASH_W, 200 + big)
    for span in (P.HASH_SPAN, P.HASH_SPAN + 1):
        # wave 1 = phrases 64 .. 127.  v sits at 15 mod 16 (v + 1 is aligned), so the wave's first byte v + a is (15 + a) mod 16
        # bytes behind its aligned-down start: span = extent of the wave + (15 + a) mod 16
        lens = [30] * 64 + [74] * 64 + [30] * 3
        a = 6 + 64 * (30 - HASH_W)
        lens[127] += span - ((15 + a) % 16) - (sum(lens[64:128]) - 63 * HASH_W)
        text, start, lens = chained_phrases(lens, HASH_W, 300 + span, first_start=6)
        assert start[64] == a and start[127] + lens[127] - a + (15 + a) % 16 == span
        out["span%d" % span] = (text, start, lens)
    return out


def route_case():
    """one content as phrase 3 (first wave: read directly), phrase 70 (a whole wave: staged in LDS) and phrase 130 (partial wave)"""
    x = rnd_text(30, 77)
    lens = [30] * 133
    return chained_phrases(lens, HASH_W, 78, fixed={3: x, 70: x, 130: x}), (3, 70, 130)


def check_phrase_hash(h1, pinfo, v, start, length, what=""):
    want_h1, want_pinfo = P.fingerprints(v, start, length)
    column(h1, want_h1, what + " h1")
    same(np.asarray(pinfo)[:len(start)], want_pinfo, what + " pinfo")
    untouched(pinfo, len(start), what + " pinfo")


def check_same_fingerprint(h1, pinfo, idx, what=""):
    """equal phrases get equal first fingerprints and equal (second fingerprint, length) fields whatever route hashed them"""
    a = idx[0]
    for b in idx[1:]:
        assert int(h1[a]) == int(h1[b]), what + ": h1 of phrases %d and %d" % (a, b)
        assert int(pinfo[a][0]) == int(pinfo[b][0]) and (int(pinfo[a][1]) & P.FP2_HI_MASK) == (int(pinfo[b][1]) & P.FP2_HI_MASK) \
            and int(pinfo[a][3]) == int(pinfo[b][3]), what + ": record fields of phrases %d and %d" % (a, b)


# ---- distinct marking -------------------------------------------------------------------------------------------------------------
RUNS = (1, 2, 64, 65, 257)                                 # equal phrases in a row: predecessors by shuffle and by lane 0's own read
RUN_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 24, 25, 33)
DIFF_AT = (0, 7, 8, 15, 16, "last")
UNIT = 40


def distinct_text():
    """a period of 40 random characters, 300 times (a phrase at s and at s + 40 k spell the same), then for every length of
    RUN_LENGTHS a base string and copies of it that differ in one byte"""
    unit = rnd_text(UNIT, 9)
    unit[5] = ord("N")
    parts = [np.tile(unit, 300)]
    variants = {}
    pos = 1 + UNIT * 300
    rng = np.random.default_rng(10)
    for l in RUN_LENGTHS:
        base = ACGT[rng.integers(0, 4, l)]
        parts.append(base); variants[(l, None)] = pos; pos += l
        for d in DIFF_AT:
            j = l - 1 if d == "last" else d
            if j >= l:
                continue
            c = base.copy()
            c[j] = ACGT[(np.flatnonzero(ACGT == c[j])[0] + 1) % 4]
            parts.append(c); variants[(l, d)] = pos; pos += l
    return np.concatenate(parts), variants


def distinct_cases():
    """name -> (text, order, h1s, pinfo).  `runs`: runs of RUNS equal phrases of RUN_LENGTHS characters, twice over (forged first
    fingerprints = run number: a run's neighbours are other phrases with another fingerprint).  `collide`: pairs with the same
    forged fingerprints and length whose bytes differ at DIFF_AT, each pair after a row of fillers so that the second of the
    pair sits at lane 1, 63 or 0 (a wave's and a workgroup's edge).  `h1_only`: equal h1, another second fingerprint."""
    text, variants = distinct_text()
    v = P.make_v(text)
    out = {}
    rec, h1s = [], []
    run_no = 0
    for rep in range(2):
        for i, cnt in enumerate(RUNS):
            l = RUN_LENGTHS[(i + 5 * rep) % len(RUN_LENGTHS)]
            off = 1 + 3 * i + rep
            for c in range(cnt):
                a = off + UNIT * (c % 290)
                rec.append(P.fingerprint(v[a:a + l], a)[1]); h1s.append(run_no)
            run_no += 1
    out["runs"] = (text, np.arange(len(rec)), K.u64(h1s), K.u32(rec))
    rec, h1s = [], []
    pairs = [(l, d) for l in RUN_LENGTHS for d in DIFF_AT if (l, d) in variants]
    key = 1
    for i, (l, d) in enumerate(pairs):
        want_lane = (1, 63, 0)[i % 3]
        while (len(rec) + 1) % 64 != want_lane:             # fillers: phrases of their own
            a = 1 + len(rec) % 200
            rec.append(P.fingerprint(v[a:a + 12], a)[1]); h1s.append(key); key += 1
        a, b = variants[(l, None)], variants[(l, d)]
        r = P.fingerprint(v[a:a + l], a)[1]
        rec.append(r); h1s.append(key)
        rec.append((r[0], r[1], b, l)); h1s.append(key); key += 1        # the base's fingerprints over other bytes
    out["collide"] = (text, np.arange(len(rec)), K.u64(h1s), K.u32(rec))
    assert len(pairs) == sum(1 for l in RUN_LENGTHS for d in DIFF_AT if d == "last" or d < l) and len(rec) > 256
    rec, h1s = [], []
    for k in range(70):
        a = 1 + k
        r = P.fingerprint(v[a:a + 20], a)[1]
        rec.append(r); h1s.append(k)
        if k in (3, 62):
            rec.append((r[0] ^ 1, r[1], r[2], r[3])); h1s.append(k)        # same text, same h1, another second fingerprint
    out["h1_only"] = (text, np.arange(len(rec)), K.u64(h1s), K.u32(rec))
    return out


def check_mark_distinct(flags, err, v, order, h1s, pinfo, what=""):
    """flags against the model; err[0] counts the collisions of both fingerprints exactly, err[1] says whether first
    fingerprints alone were shared, the rest of err is untouched"""
    want, e0, e1 = P.mark_distinct(order, h1s, pinfo, v)
    column(flags, want, what + " flags")
    assert int(err[0]) == e0, what + ": err[0] = %d, expected %d collisions of both fingerprints" % (int(err[0]), e0)
    assert int(err[1]) == e1, what + ": err[1] = %d, expected %d" % (int(err[1]), e1)
    untouched(err, 2, what + " err")


# ---- dictionary -------------------------------------------------------------------------------------------------------------------
COPY_LENGTHS = (1, 63, 64, 65)                             # one wave copies a phrase 64 bytes a step


def copy_case(seed=3):
    """(text, start, len, which, dstart, dict_len): phrases of COPY_LENGTHS characters, twice, copied in another order; phrase 0
    starts at V index 0 (Dollar)"""
    text = rnd_text(600, seed)
    text[100] = ord("N")
    lens = list(COPY_LENGTHS) * 2
    start = [0, 5, 90, 200, 300, 310, 400, 470]
    which = [3, 0, 7, 1, 2, 6, 5, 4]
    dlen = [lens[p] + 1 for p in which]
    dstart = np.cumsum([0] + dlen[:-1]).tolist()
    return text, start, lens, which, dstart, sum(dlen) + 1


def check_copy_dict(d, info, v, start, lens, which, dstart, dict_len, pack_prev, tripped=None, what=""):
    """dictionary bytes and records against the model; a phrase whose offset trips the guard (tripped = its index in `which`,
    copied to true_dstart in the model) leaves its bytes untouched"""
    want_d, want_i = P.copy_dict(v, start, lens, which, dstart if tripped is None else tripped[1], dict_len, pack_prev)
    want_d = want_d.copy(); want_i = want_i.copy()
    keep = np.ones(dict_len, bool)
    if tripped is not None:
        k, true_dstart = tripped
        keep[true_dstart[k]:true_dstart[k] + lens[which[k]] + 1] = False
    got_d = np.asarray(d)[:dict_len]
    same(got_d[keep], want_d[keep], what + " dict")
    assert np.all(got_d[~keep] == K.SENT8), what + ": bytes of the refused phrase were written"
    untouched(d, dict_len, what + " dict")
    if info is not None:
        got_i = np.asarray(info)[:dict_len]
        same(got_i[keep], want_i[keep], what + " dinfo")
        assert np.all(got_i[~keep] == U64(K.SENT64)), what + ": records of the refused phrase were written"
        untouched(info, dict_len, what + " dinfo")


ENTRY_ND = (1, 3, 4, 5, 7, 8)                              # four entries per work-item: the vector path and the tail


def entry_case(nd, seed=4):
    """a forged dictionary of nd bytes with a Dollar in it, records with every field in use, a suffix array that holds position 0"""
    rng = np.random.default_rng(seed + nd)
    d = rng.integers(3, 90, nd).astype(U8)
    if nd > 2:
        d[1] = 2                                           # the byte before position 2 is Dollar: bwt 0
    info = rng.integers(0, 1 << 63, nd, dtype=np.int64).astype(U64)
    if nd > 3:
        info[3] = (U64(2) << U64(56)) | (info[3] & U64((1 << 56) - 1))      # packed form: a Dollar in the top byte
    return d, info, rng.permutation(nd).astype(U32)


def check_entry_info(esuf, ephr, ebw, sa_d, d, info, pack_prev, what=""):
    we, wp, wb = P.entry_info(sa_d, d, info, pack_prev)
    column(esuf, we, what + " esuf"); column(ephr, wp, what + " ephr"); column(ebw, wb, what + " ebw")


# ---- dictionary LCP ---------------------------------------------------------------------------------------------------------------
SHARED = (127, 128, 129, 135, 136)                         # k_dict_irr compares 16 x 8 = 128 characters before the long list
EXACT_LIMIT = 200                                          # a phrase that is a prefix of another: the match ends at the limit


def lcp_dictionary(seed=6):
    """a forged dictionary (through the model's copy_dict): pairs of phrases that share SHARED characters, a phrase of
    EXACT_LIMIT characters that is a prefix of another, one of 128 that is, and short phrases"""
    rng = np.random.default_rng(seed)
    phrases = []
    for s in SHARED:
        c = ACGT[rng.integers(0, 4, s)]
        phrases.append(np.concatenate([c, [ord("A")], ACGT[rng.integers(0, 4, 9)]]))
        phrases.append(np.concatenate([c, [ord("C")], ACGT[rng.integers(0, 4, 14)]]))
    for lim in (EXACT_LIMIT, P.DICT_IRR_CHARS):
        c = ACGT[rng.integers(0, 4, lim)]
        phrases.append(c)
        phrases.append(np.concatenate([c, [ord("G")], ACGT[rng.integers(0, 4, 5)]]))
    for _ in range(6):
        phrases.append(ACGT[rng.integers(0, 4, int(rng.integers(1, 20)))])
    order = rng.permutation(len(phrases))
    phrases = [phrases[i] for i in order]
    text = np.concatenate(phrases)
    lens = [len(x) for x in phrases]
    start = (1 + np.cumsum([0] + lens[:-1])).tolist()
    dlen = [l + 1 for l in lens]
    dstart = np.cumsum([0] + dlen[:-1]).tolist()
    nd = sum(dlen) + 1
    d, info = P.copy_dict(P.make_v(text), start, lens, list(range(len(lens))), dstart, nd, False)
    sa_d = P.dict_suffix_array(d)
    esuf, ephr, ebw = P.entry_info(sa_d, d, info)
    return d, sa_d, esuf, ebw


def check_dict_irreducible(plcp, longs, count, long_cap, d, sa_d, esuf, ebw, what=""):
    """plcp of the entries decided in the kernel, the true number of long pairs in long_count, long_cap records of the model's
    set (in any order, no two alike) and nothing behind them"""
    first, want_longs, _ = P.dict_irreducible(d, sa_d, esuf, ebw)
    mask = np.ones(len(first), bool)
    for p, q, h, lim in want_longs:
        mask[p] = False                                    # (left for long_lcp_lim)
    same(np.asarray(plcp)[mask], first[mask], what + " plcp")
    same(np.asarray(plcp)[~mask], np.zeros(int((~mask).sum()), U32), what + " plcp of the long entries")
    assert count == len(want_longs), what + ": long_count %d, expected %d" % (count, len(want_longs))
    wrote = min(count, long_cap)
    got = [tuple(int(x) for x in r) for r in np.asarray(longs)[:wrote]]
    assert len(set(got)) == wrote and set(got) <= want_longs, what + ": long records " + repr(got)
    untouched(longs, wrote, what + " longs")


def check_dict_lcp(lcp, d, sa_d, esuf, what=""):
    column(lcp, P.naive_dict_lcp(d, sa_d, esuf), what + " lcp_d")


# ---- group tables -------------------------------------------------------------------------------------------------------------------
GROUP_W = 5


def group_case():
    """forged (esuf, lcp_d) for w = 5: suffixes of 4, 5 and 6 characters, phrase starts in between, neighbours of equal length
    with lcp = len - 1, len and len + 1, a valid entry at r = 0"""
    S = 0x80000000
    esuf = [6, 6, 6, 6, S | 9, 4, 5, 5, S | 5, 5, 6, 0, 7, 7, S | 7, 7, 7, 4, 4, 0]
    lcp = [3, 5, 6, 7, 2, 4, 4, 5, 5, 5, 5, 0, 0, 8, 7, 7, 6, 4, 4, 0]
    return K.u32(esuf), K.u32(lcp)


def check_group_flags(g, p, v, seg, esuf, lcp, w, what=""):
    wg, wp, wv, ws = P.group_flags(esuf, lcp, w)
    column(g, wg, what + " gflag"); column(p, wp, what + " pflag"); column(v, wv, what + " vflag"); column(seg, ws, what + " seg")


# ---- inverted lists -----------------------------------------------------------------------------------------------------------------
OCC_M = (1, 2, 65)
SL_EDGES = (0xFFFFFE, 0xFFFFFF, 0x1000000)                 # occ_finish12 keeps 24 bits of sl and saturates at 0xffffff


def occ_case(m, first, wide, seed=8):
    """a forged parse of m phrases over D = 5 distinct ones; `first` (0 lowest, 1 middle, 2 highest id) moves the rank of the
    parse's first suffix; pstart ascends (wide: above 2^32, high byte 0xff); sl holds SL_EDGES; pos_bits puts the largest t on
    bit 63"""
    rng = np.random.default_rng(seed + m)
    D = 5
    pid = rng.integers(1, D - 1, m).astype(U32)
    pid[0] = (0, 2, D - 1)[first]
    sa_p = K.ref_suffix_array(pid.astype(np.int64) + 1)
    base = (0xFF << 32) if wide else 0
    pstart = [base + 7 + 11 * q for q in range(m)]
    sl = rng.integers(0, 1 << 20, m).astype(U32)
    for i, x in enumerate(SL_EDGES):
        if i + 1 < m:
            sl[i + 1] = x
    sl[0] = 0
    pos_bits = 64 - m.bit_length()
    assert (m << pos_bits) >> 63 == 1 and pstart[-1] < (1 << pos_bits)
    return pid, sa_p, pstart, sl, D, pos_bits


def check_occ_sequence(keys, vals, sa_p, pid, D, what=""):
    wk, wv = P.occ_sequence(sa_p, pid, D)
    column(keys, wk, what + " keys"); column(vals, wv, what + " vals")


def check_occ_finish(mode, occ_start, occ, occ_sl, ids, ts, sa_p, pstart, sl, pos_bits, what=""):
    m = len(sa_p)
    ws, wo, wsl, w12 = P.occ_lists(ids, ts, sa_p, pstart, sl, pos_bits, len(occ_start))
    for i, x in enumerate(ws):
        assert int(occ_start[i]) == (K.SENT32 if x is None else x), what + ": occ_start[%d] = %d, expected %s" % (i, int(occ_start[i]), x)
    assert ws[int(ids[m])] == m, what + ": the dummy's list begins at m"
    if mode == 8:
        column(occ, wo, what + " occ"); column(occ_sl, wsl, what + " occ_sl")
    else:
        same(np.asarray(occ)[:m], w12, what + " occ12"); untouched(occ, m, what + " occ12")


# ---- emitter bookkeeping ----------------------------------------------------------------------------------------------------------------
def oversize_case(wide):
    """groups of EMIT_CAP - 1, EMIT_CAP and EMIT_CAP + 1 = 1023, 1024, 1025 suffixes, small ones, and (wide) one of 2^32"""
    sizes = [3, P.EMIT_CAP - 1, P.EMIT_CAP, P.EMIT_CAP + 1, 1, 5000]
    if wide:
        sizes += [1 << 32, 0xFFFFFFFF, 0xFFFFFFFE, 7]
    return np.cumsum([9] + sizes).tolist()


def check_oversize(osize, err, segb, what=""):
    want, big = P.oversize(segb)
    column(osize, want, what + " osize")
    assert int(err[2]) == big and int(err[0]) == 0 and int(err[1]) == 0, what + ": err = %s, expected err[2] = %d" % (err[:3], big)
    untouched(err, 3, what + " err")


def tile_case(tile, wide):
    """group begins around the tile edges: groups inside tile 0, none in tiles 1 and 2, one exactly on the edge of tile 3, one
    just before and one just behind the edge of tile 4"""
    base = (1 << 32) // tile * tile if wide else 0
    return [base + x for x in (0, 5, tile - 1, 3 * tile, 4 * tile - 1, 4 * tile + 1, 5 * tile + 7)], base // tile


# ---- parse LCP ------------------------------------------------------------------------------------------------------------------------
PARSE_W, PARSE_P = 4, 11
PARSE_M = (1, 2, 64, 65, 4097)
PARSE_SHARED = (63, 64, 65, 511, 512, 513)                 # k_parse_cmp: 64 characters a step, CMP_STEPS x 64 = 512 before the long list


def trigger_word(w, p, seed=12):
    """w characters whose window fingerprint is a multiple of p: a phrase ends behind them wherever they stand"""
    rng = np.random.default_rng(seed)
    while True:
        x = ACGT[rng.integers(0, 4, w)]
        if int(P.kr_hashes(x, w)[-1]) % p == 0:
            return x


def text_of_m_phrases(m, w, p, seed=13):
    """a random text cut right behind its (m - 1)-th trigger: exactly m phrases"""
    if m == 1:
        t = rnd_text(40, seed)
        while len(P.triggers(t, w, p)):
            seed += 1; t = rnd_text(40, seed)
        return t
    n = 64
    while True:
        t = rnd_text(n, seed + m)
        cuts = P.triggers(t, w, p)
        if len(cuts) >= m - 1:
            return t[:int(cuts[m - 2]) + 1]
        n *= 2


def shared_text(w=PARSE_W, p=PARSE_P, seed=14):
    """Pairs of phrase starts whose suffixes share exactly PARSE_SHARED characters (the trigger word, a string of their own,
    then different characters), and for every pair (i, j) of offsets mod 8 a pair that shares 20 + i + j and starts at i and j"""
    rng = np.random.default_rng(seed)
    tw = trigger_word(w, p)
    parts, pos = [], 0

    def filler(k):
        return ACGT[rng.integers(0, 4, k)]

    def put(x):
        nonlocal pos
        parts.append(np.asarray(x, dtype=U8)); pos += len(x)

    def pair(share, mod_a=None, mod_b=None):
        own = filler(share - w)
        for tail, mod in ((ord("A"), mod_a), (ord("C"), mod_b)):
            k = 12 + int(rng.integers(0, 8))
            if mod is not None:
                k = 12 + (mod - (pos + 12)) % 8
            put(filler(k)); assert mod is None or pos % 8 == mod
            put(tw); put(own); put([tail]); put(filler(3))

    for s in PARSE_SHARED:
        pair(s)
    for i in range(8):
        for j in range(8):
            pair(20 + i + j, i, j)
    put(filler(30))
    return np.concatenate(parts)


def identical_haplotypes(w=PARSE_W, p=PARSE_P, seed=15):
    h = rnd_text(1500, seed)
    return np.concatenate([h, [ord("$")], h, [ord("$")], h, [ord("$")]])


def check_parse_lcp(sl, bmin, nb, levels, n_irr, n_long, M, what=""):
    """sl against its definition, every level of the block minima, the counts of irreducible and of long pairs"""
    same(sl, M.sl, what + " sl")
    assert (nb, levels) == (M.nb, M.levels), what + ": nb, levels = %d, %d, expected %d, %d" % (nb, levels, M.nb, M.levels)
    column(bmin, M.bmin, what + " bmin")
    assert n_irr == M.n_irreducible, what + ": n_irreducible %d, expected %d" % (n_irr, M.n_irreducible)
    assert n_long == M.n_long, what + ": n_long %d, expected %d" % (n_long, M.n_long)


# ---- RMQ ------------------------------------------------------------------------------------------------------------------------------
RMQ_BUILD_M = (1, 63, 64, 65, 127, 128, 129, 4096, 4097)


def check_build_rmq(nb, levels, bmin, vals, what=""):
    wn, wl, wb = P.rmq_tables(vals)
    assert (nb, levels) == (wn, wl), what + ": nb, levels = %d, %d, expected %d, %d" % (nb, levels, wn, wl)
    column(bmin, wb, what + " bmin")


def rmq_pairs_all(m=300):
    return [(a, b) for a in range(m) for b in range(a, m)]


def rmq_pairs_edges(m=10000):
    """b - a = 127, 128, 129 (the scan ends at b - a = 128) with a and b on, just before and just behind multiples of 64; a = 0
    and b = m - 1; long ranges"""
    out = set()
    for d in (127, 128, 129):
        for base in range(0, m, 64):
            for x in (base - 1, base, base + 1):
                for a, b in ((x, x + d), (x - d, x)):
                    if 0 <= a <= b < m:
                        out.add((a, b))
        out.add((0, d)); out.add((m - 1 - d, m - 1))
    for a, b in ((0, m - 1), (0, 63), (0, 64), (1, m - 1), (63, m - 2), (64, m - 65), (65, 5000), (4999, 5130)):
        out.add((a, b))
    return sorted(out)


def rmq_min_places(a, b):
    """where a range's only minimum is put in turn: the head stretch (before the first whole block), the tail stretch, the
    first whole block, the last whole block, the middle"""
    ba, bb = (a + 63) >> 6, (b + 1) >> 6
    places = [a, b, ba * 64 + 5, bb * 64 - 5, (a + b) // 2]
    if a < ba * 64:
        places.append(ba * 64 - 1)
    if bb * 64 <= b:
        places.append(bb * 64)
    return [x for x in places if a <= x <= b]


def check_rmq(out, out8, vals, pairs, what=""):
    want = P.rmq_answers(vals, pairs)
    same(out, want, what + " rmq_min")
    same(out8, want, what + " rmq_min8")
