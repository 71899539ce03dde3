"""A CPU model of the tables of the prefix-free parse (csrc/pfp_kernels.hip rows A2-A4, csrc/parse_lcp.hip): given (T, w, p)
every array the launch wrappers read or write, stage by stage and in product order (csrc/pfp.cpp: pfp_parse, then
pfp_prepare_emitter / pfp_group_tables).  Plain Python and numpy, integers only, Python ints wherever 64 bits could
overflow; nothing is imported from the product.  tests/test_pfp_model_host.py holds the model to independent statements
(the reference parser's golden files, a rolling Karp-Rabin, the oracle's parse, naive suffix and LCP computations), so that
a broken model cannot make a GPU test pass vacuously.

The stage functions take their inputs as arguments (the GPU tests feed forged inputs through the same functions); Model
chains them for a real text."""
import numpy as np

import kprobe as K

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
M64 = (1 << 64) - 1
KR_PRIME = 1999999973                     # pfp_kernels.hpp
B1, B2 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F
LEN_MIX = 0xD6E8FEB86659FD93
FP2_HI_MASK = 0x00FFFFFF
HASH_SPAN = 4096
HASH_LONG = 2048                          # phrases longer than this are hashed by the whole wave
LCP_CAP = 0xFFF00000                      # wide.hpp
EMIT_CAP = 1024
DICT_IRR_CHARS = 16 * 8                   # k_dict_irr hands over to the long list behind 128 equal characters
PARSE_CMP_CHARS = 8 * 64                  # k_parse_cmp: CMP_STEPS x 64 = 512
RMQ_SCAN = 128                            # rmq_min scans ranges with b - a < 128


def make_v(text, pad=64):
    """V = Dollar . T . Dollar^32 . zeros (the byte layout of textref.hpp; pad >= 64)"""
    text = K.u8(text)
    return np.concatenate([np.full(1, 2, U8), text, np.full(32, 2, U8), np.zeros(pad, U8)])


# ---- parse front --------------------------------------------------------------------------------------------------------
def kr_hashes(text, w):
    """h[i] = sum_{k < w} T[i - k] 256^k mod KR_PRIME, T[< 0] = 0: the fingerprint of the window that ends at i"""
    t = np.asarray(text, dtype=np.int64)
    n = len(t)
    acc = np.zeros(n, np.int64)
    for k in range(min(w, n)):
        term = np.zeros(n, np.int64)
        term[k:] = t[:n - k] * pow(256, k, KR_PRIME)      # < 256 * 2^31: 32 such terms fit 63 bits
        acc += term
    return acc % KR_PRIME


def triggers(text, w, p, hashes=None):
    """positions i with i + 1 >= w and h[i] % p == 0, ascending"""
    h = kr_hashes(text, w) if hashes is None else hashes
    i = np.arange(len(h), dtype=np.int64)
    return np.flatnonzero((h % p == 0) & (i + 1 >= w))


def trigger_blocks(n):
    return max(1, ((n + 15) // 16 + 255) // 256)


def trigger_masks(n, cuts):
    """(masks: bit q of masks[t] = trigger at 16 t + q, ceil(n / 16) entries; block_count: triggers per 4096 positions)"""
    bits = np.zeros(((n + 15) // 16) * 16, np.int64)
    bits[np.asarray(cuts, dtype=np.int64)] = 1
    masks = (bits.reshape(-1, 16) << np.arange(16)).sum(axis=1).astype(U16)
    per = np.zeros(trigger_blocks(n) * 4096, np.int64)
    per[:len(bits)] = bits
    return masks, per.reshape(-1, 4096).sum(axis=1).astype(U32)


def cuts_of_masks(masks, n):
    """trigger positions spelled by a (forged) mask array"""
    out = []
    for t in range((n + 15) // 16):
        for q in range(16):
            if (int(masks[t]) >> q) & 1:
                out.append(16 * t + q)
    return out


def phrase_bounds(cuts, n, w):
    """phrase k = V[start[k] .. start[k] + len[k]): from the window of the cut before it (V index 0 for the first) up to and
    including the window of its own cut (the last phrase: up to the w Dollars behind the text).  Python ints."""
    cuts = [int(c) for c in cuts]
    start = [0] + [c - w + 2 for c in cuts]
    last = [c + 1 for c in cuts] + [n + w]
    return start, [b - a + 1 for a, b in zip(start, last)]


# ---- fingerprints -------------------------------------------------------------------------------------------------------
def poly(chars, base):
    h = 0
    for c in chars:
        h = (h * base + int(c) + 1) & M64
    return h


def fingerprint(chars, start):
    """(h1, pinfo record) of a phrase with these characters at V index `start`"""
    l = len(chars)
    h1 = poly(chars, B1) ^ ((l * LEN_MIX) & M64)
    g2 = (poly(chars, B2) + (l << 32)) & M64
    return h1, (g2 & 0xFFFFFFFF, ((g2 >> 32) & FP2_HI_MASK) | (((start >> 32) & 0xFF) << 24), start & 0xFFFFFFFF, l)


def fingerprints(v, start, length):
    h1 = np.empty(len(start), U64)
    pinfo = np.empty((len(start), 4), U32)
    for k, (a, l) in enumerate(zip(start, length)):
        h1[k], rec = fingerprint(v[a:a + l], a)
        pinfo[k] = rec
    return h1, pinfo


def second_fingerprint(pinfo):
    pinfo = np.asarray(pinfo, dtype=U64).reshape(-1, 4)
    return ((pinfo[:, 1] & U64(FP2_HI_MASK)) << U64(32)) | pinfo[:, 0]


def record_start(rec):
    return ((int(rec[1]) >> 24) << 32) | int(rec[2])


# ---- distinct phrases ----------------------------------------------------------------------------------------------------
def mark_distinct(order, h1s, pinfo, v):
    """flags[k] = 0 iff entry k spells the phrase of entry k - 1: equal first fingerprint, equal second fingerprint and
    length, equal bytes.  err0 = entries with both fingerprints and the length equal but other bytes; err1 = 1 when two
    neighbours share the first fingerprint and differ in the second or the length."""
    m = len(order)
    flags = np.ones(m, U32)
    err0 = err1 = 0
    for k in range(1, m):
        if int(h1s[k]) != int(h1s[k - 1]):
            continue
        x, y = pinfo[order[k]], pinfo[order[k - 1]]
        if int(x[0]) != int(y[0]) or (int(x[1]) & FP2_HI_MASK) != (int(y[1]) & FP2_HI_MASK) or int(x[3]) != int(y[3]):
            err1 = 1
            continue
        a, b, l = record_start(x), record_start(y), int(x[3])
        if np.array_equal(v[a:a + l], v[b:b + l]):
            flags[k] = 0
        else:
            err0 += 1
    return flags, err0, err1


def assign_distinct(order, flags, length):
    scan = np.cumsum(np.asarray(flags, dtype=np.int64))
    m, d = len(order), int(scan[-1])
    pid = np.empty(m, U32); rep = np.empty(d, U32); dlen = np.empty(d, U32)
    for k in range(m):
        pid[order[k]] = scan[k] - 1
        if flags[k]:
            rep[scan[k] - 1] = order[k]
            dlen[scan[k] - 1] = length[order[k]] + 1
    return scan.astype(U32), pid, rep, dlen


# ---- dictionary ------------------------------------------------------------------------------------------------------------
def copy_dict(v, start, length, which, dstart, dict_len, pack_prev):
    """(dict, dinfo): phrase bytes, 0x01 behind every phrase, 0x00 at the very end.  dinfo[pos] = (id << 32) | (length of the
    phrase suffix at pos, 0 on terminators, bit 31 on a phrase's first byte); pack_prev: the byte before pos in bits 56..63
    (the terminator 0x01 before a phrase's first byte, 0 before the first phrase)."""
    d = np.zeros(dict_len, U8)
    info = [0] * dict_len
    for k, ph in enumerate(which):
        a, l, o = int(start[ph]), int(length[ph]), int(dstart[k])
        d[o:o + l] = v[a:a + l]
        d[o + l] = 1
        for i in range(l + 1):
            word = 0 if i == l else (l - i) | (0x80000000 if i == 0 else 0)
            prev = (int(v[a + i - 1]) if i else (1 if k else 0)) if pack_prev else 0
            info[o + i] = (prev << 56) | (k << 32) | word
    k = len(which) - 1
    d[dict_len - 1] = 0
    info[dict_len - 1] = ((1 << 56) if pack_prev else 0) | (k << 32)
    return d, np.array(info, dtype=U64)


def dict_suffix_array(d):
    """a plain sort of the dictionary suffixes; 0x01 and 0x00 end a suffix and are symbols of their own (ordered by
    position, below every other byte)"""
    sym = np.where(np.asarray(d) <= 1, 0, np.asarray(d)).astype(np.int64)
    return K.ref_suffix_array(sym, terminator=0)


def entry_info(sa_d, d, dinfo, pack_prev=False):
    """esuf (suffix word), ephr (distinct id) and ebw (the byte before the suffix; 0 at position 0 and for Dollar).
    pack_prev: the id is 24 bits and the byte before rides in bits 56..63 of the record; else it is read from the dictionary."""
    pos = np.asarray(sa_d, dtype=np.int64)
    e = np.asarray(dinfo, dtype=U64)[pos]
    if pack_prev:
        prev = (e >> U64(56)).astype(U8)
        ephr = ((e >> U64(32)) & U64(0xFFFFFF)).astype(U32)
    else:
        prev = np.where(pos > 0, np.asarray(d)[np.maximum(pos - 1, 0)], 0).astype(U8)
        ephr = (e >> U64(32)).astype(U32)
    prev[prev == 2] = 0
    return (e & U64(0xFFFFFFFF)).astype(U32), ephr, prev


def naive_dict_lcp(d, sa_d, esuf):
    """lcp_d[r] = common characters of the phrase suffixes at sa_d[r - 1] and sa_d[r] (a match ends with the shorter one)"""
    nd = len(sa_d)
    sl = np.asarray(esuf, dtype=np.int64) & 0x7FFFFFFF
    out = np.zeros(nd, U32)
    for r in range(1, nd):
        a, b, lim = int(sa_d[r - 1]), int(sa_d[r]), int(min(sl[r - 1], sl[r]))
        x, y = d[a:a + lim], d[b:b + lim]
        ne = np.flatnonzero(x != y)
        out[r] = ne[0] if len(ne) else lim
    return out


def dict_irreducible(d, sa_d, esuf, ebw):
    """(plcp after dict_irreducible, the long records as a set of (p, q, h, lim), plcp after long_lcp_lim)"""
    nd = len(sa_d)
    sl = np.asarray(esuf, dtype=np.int64) & 0x7FFFFFFF
    st = np.asarray(esuf, dtype=np.int64) >> 31
    lcp = naive_dict_lcp(d, sa_d, esuf)
    first = np.zeros(nd, U32); full = np.zeros(nd, U32)
    longs = set()
    for r in range(1, nd):
        lim = int(min(sl[r], sl[r - 1]))
        if lim > 0 and (st[r] or st[r - 1] or ebw[r] != ebw[r - 1]):
            p = int(sa_d[r])
            full[p] = lcp[r]
            if lim > DICT_IRR_CHARS and int(lcp[r]) >= DICT_IRR_CHARS:
                longs.add((p, int(sa_d[r - 1]), DICT_IRR_CHARS, lim))
            else:
                first[p] = lcp[r]
    return first, longs, full


def plcp_running_max(plcp):
    i = np.arange(len(plcp), dtype=np.int64)
    return (np.maximum.accumulate(np.asarray(plcp, dtype=np.int64) + i) - i).astype(U32)


def dict_lcp_clamp(lcp, esuf):
    sl = np.asarray(esuf, dtype=np.int64) & 0x7FFFFFFF
    before = np.concatenate([[0], sl[:-1]])
    out = np.minimum(np.asarray(lcp, dtype=np.int64), np.minimum(sl, before))
    out[0] = 0
    return out.astype(U32)


# ---- groups and ranks --------------------------------------------------------------------------------------------------------
def group_flags(esuf, lcp_d, w):
    """valid = a proper phrase suffix of w characters or more; gflag = valid and not the same string as the valid entry before
    (same length, all of it shared); pflag = first byte of a phrase; seg = (entry before valid, or r = 0) << 32 | lcp"""
    e = np.asarray(esuf, dtype=np.int64)
    sl, st = e & 0x7FFFFFFF, e >> 31
    valid = (st == 0) & (sl >= w)
    pvalid = np.concatenate([[False], valid[:-1]])
    psl = np.concatenate([[0], sl[:-1]])
    l = np.asarray(lcp_d, dtype=np.int64)
    same = valid & pvalid & (psl == sl) & (l >= sl)
    head = pvalid.copy(); head[0] = True
    seg = (head.astype(U64) << U64(32)) | l.astype(U64)
    return (valid & ~same).astype(U32), st.astype(U32), valid.astype(U32), seg


def segmin(seg):
    """inclusive segmented minimum: (flag of the segment's head, minimum of the values from that head on)"""
    out = np.empty(len(seg), U64)
    cur = None
    for i, x in enumerate(seg):
        x = int(x)
        if (x >> 32) or cur is None:
            cur = x
        else:
            cur = (cur & ~0xFFFFFFFF) | min(cur & 0xFFFFFFFF, x & 0xFFFFFFFF)
        out[i] = cur
    return out


def phrase_ranks(esuf, ephr, pflag, n_distinct):
    pscan = np.cumsum(np.asarray(pflag, dtype=np.int64)).astype(U32)
    prank = np.zeros(n_distinct, U32)
    st = (np.asarray(esuf, dtype=np.int64) >> 31) == 1
    prank[np.asarray(ephr)[st]] = pscan[st]
    return pscan, prank


def invert_ranks(prank, rep, dlen):
    which = np.empty(len(prank), U32); slen = np.empty(len(prank), U32)
    which[np.asarray(prank, dtype=np.int64) - 1] = rep
    slen[np.asarray(prank, dtype=np.int64) - 1] = dlen
    return which, slen


# ---- inverted lists ------------------------------------------------------------------------------------------------------------
def occ_sequence(sa_p, pid, n_distinct):
    """keys[0] = the parse's last phrase, keys[r + 1] = the phrase before parse suffix sa_p[r] (the dummy id D before the
    first); vals[t] = t"""
    m = len(sa_p)
    keys = np.empty(m + 1, U32)
    keys[0] = pid[m - 1]
    q = np.asarray(sa_p, dtype=np.int64)
    keys[1:] = np.where(q > 0, np.asarray(pid)[np.maximum(q - 1, 0)], n_distinct)
    return keys, np.arange(m + 1, dtype=U32)


def occ_lists(ids, ts, sa_p, pstart, sl, pos_bits, n_start):
    """occ_start[id] = first k of id (others untouched: None); per k < m: t, V start of the occurrence, sl[t - 1]"""
    m = len(sa_p)
    occ_start = [None] * n_start
    for k in range(m + 1):
        if k == 0 or ids[k] != ids[k - 1]:
            occ_start[int(ids[k])] = k
    t = [int(x) for x in ts[:m]]
    pos = [int(pstart[int(sa_p[x - 1]) - 1 if x else m - 1]) for x in t]
    osl = [int(sl[x - 1]) if x else 0 for x in t]
    occ = np.array([((x << pos_bits) | q) & M64 for x, q in zip(t, pos)], dtype=U64)
    occ12 = np.array([[x, q & 0xFFFFFFFF, ((q >> 32) & 0xFF) | (min(s, 0xFFFFFF) << 8)] for x, q, s in zip(t, pos, osl)],
                     dtype=U64).astype(U32).reshape(-1, 3)
    return occ_start, occ, np.array(osl, dtype=U32), occ12


def phrase_table(occ_start, plen, rep):
    d = len(rep)
    os_ = np.asarray(occ_start, dtype=np.int64)
    tab = np.zeros((d, 4), U32)
    tab[:, 0] = os_[1:d + 1] - os_[:d]; tab[:, 1] = os_[:d]; tab[:, 2] = np.asarray(plen)[np.asarray(rep, dtype=np.int64)]
    return tab


def entry_compact(esuf, ephr, ebw, gflag, vflag, seg_min, tab):
    """the valid entries, compacted: occurrences and first list slot of the entry's phrase, offset inside the phrase minus one,
    BWT byte, g + 1 at the first entry of group g (else 0), LCP with the valid entry before, suffix length"""
    v = np.flatnonzero(np.asarray(vflag))
    gscan = np.cumsum(np.asarray(gflag, dtype=np.int64))
    vscan = np.cumsum(np.asarray(vflag, dtype=np.int64)) - np.asarray(vflag, dtype=np.int64)
    sl = (np.asarray(esuf, dtype=np.int64) & 0x7FFFFFFF)[v]
    t = np.asarray(tab, dtype=np.int64)[np.asarray(ephr, dtype=np.int64)[v]]
    ce = dict(cnt=t[:, 0].astype(U32), first=t[:, 1].astype(U32), offm1=(t[:, 2] - sl - 1).astype(U32), bwt=np.asarray(ebw)[v].astype(U8),
              gs=np.where(np.asarray(gflag)[v] != 0, gscan[v], 0).astype(U32),
              hl=(np.asarray(seg_min, dtype=U64)[v] & U64(0xFFFFFFFF)).astype(U32), slen=sl.astype(U32))
    return gscan.astype(U32), vscan.astype(U32), ce


def group_heads(sege, ce_hl, ce_slen):
    g = len(sege)
    out = np.zeros((g, 2), U32)
    for i in range(g):
        e = int(sege[i])
        la = int(ce_slen[e])
        out[i] = (la, min(int(ce_hl[e]), la, int(ce_slen[e - 1])) if i else 0)
    return out


def tile_first(segb, tiles, tile, tile_base=0):
    """out[t - tile_base] = first group whose begin offset is >= t * tile (n_groups when none), t = tile_base .. tiles"""
    segb = [int(x) for x in segb]
    return K.u32([next((g for g, b in enumerate(segb) if b >= t * tile), len(segb)) for t in range(tile_base, tiles + 1)])


def oversize(segb):
    sz = [int(segb[g + 1]) - int(segb[g]) for g in range(len(segb) - 1)]
    return K.u32([s & 0xFFFFFFFF if s > EMIT_CAP else 0 for s in sz]), sum(1 for s in sz if s >= 0xFFFFFFFF)


# ---- parse LCP ---------------------------------------------------------------------------------------------------------------
def common_prefix(v, a, b, limit):
    x, y = v[a:a + limit], v[b:b + limit]
    ne = np.flatnonzero(x != y)
    return int(ne[0]) if len(ne) else limit


def parse_sl(v, nv, sa_p, pstart):
    """sl[r] = equal characters of V from pstart[sa_p[r]] and from pstart[sa_p[r - 1]], bounded by the room up to nv and by
    LCP_CAP; sl[0] = 0"""
    m = len(sa_p)
    sl = np.zeros(m, U32)
    for r in range(1, m):
        a, b = int(pstart[sa_p[r]]), int(pstart[sa_p[r - 1]])
        sl[r] = common_prefix(v, a, b, min(nv - max(a, b), LCP_CAP))
    return sl


def parse_irreducible(v, nv, sa_p, pid, pstart):
    """(number of irreducible entries r >= 1 -- one of the two suffixes starts the parse or the phrases before them differ --,
    number of those that share PARSE_CMP_CHARS characters and have room for more: the long list)"""
    n_irr = n_long = 0
    for r in range(1, len(sa_p)):
        qa, qb = int(sa_p[r]), int(sa_p[r - 1])
        if qa == 0 or qb == 0 or pid[qa - 1] != pid[qb - 1]:
            n_irr += 1
            a, b = int(pstart[qa]), int(pstart[qb])
            limit = min(nv - max(a, b), LCP_CAP)
            if limit > PARSE_CMP_CHARS and common_prefix(v, a, b, PARSE_CMP_CHARS) == PARSE_CMP_CHARS:
                n_long += 1
    return n_irr, n_long


def rmq_tables(vals):
    """(nb, levels, bmin): minima of blocks of 64, then level k = minimum of blocks [b, b + 2^k) (blocks past the end count as
    0xffffffff)"""
    vals = K.u32(vals); m = len(vals)
    nb = (m + 63) // 64
    levels = 1
    while (1 << levels) <= nb:
        levels += 1
    padded = np.full(nb * 64, 0xFFFFFFFF, U32); padded[:m] = vals
    rows = [padded.reshape(nb, 64).min(axis=1)]
    for k in range(1, levels):
        half = 1 << (k - 1)
        shifted = np.full(nb, 0xFFFFFFFF, U32); shifted[:max(nb - half, 0)] = rows[-1][half:]
        rows.append(np.minimum(rows[-1], shifted))
    return nb, levels, np.concatenate(rows)


def rmq_answers(vals, pairs):
    vals = K.u32(vals)
    return K.u32([vals[a:b + 1].min() for a, b in pairs])


# ---- the whole chain ---------------------------------------------------------------------------------------------------------
class Model:
    """every table of the parse of T with (w, p), in product order"""

    def __init__(self, text, w, p, with_lists=True):
        self.text = K.u8(text); self.n = n = len(self.text); self.w = w; self.p = p
        self.v = v = make_v(self.text)
        self.nv = n + 1 + w
        self.cuts = triggers(self.text, w, p)
        self.masks, self.block_count = trigger_masks(n, self.cuts)
        self.pstart, self.plen = phrase_bounds(self.cuts, n, w)
        self.m = m = len(self.pstart)
        self.h1, self.pinfo = fingerprints(v, self.pstart, self.plen)
        self.order = np.argsort(self.h1, kind="stable").astype(U32)
        self.h1s = self.h1[self.order]
        self.dflags, self.err0, self.err1 = mark_distinct(self.order, self.h1s, self.pinfo, v)
        self.scan, self.pid, self.rep, self.dlen = assign_distinct(self.order, self.dflags, self.plen)
        self.D = D = len(self.rep)
        self.dstart = (np.cumsum(self.dlen.astype(np.int64)) - self.dlen).astype(U32)
        self.dict_len = nd = int(self.dlen.astype(np.int64).sum()) + 1
        self.dict, self.dinfo_packed = copy_dict(v, self.pstart, self.plen, self.rep, self.dstart, nd, True)
        _, self.dinfo_plain = copy_dict(v, self.pstart, self.plen, self.rep, self.dstart, nd, False)
        self.sa_d = dict_suffix_array(self.dict)
        self.esuf, self.ephr, self.ebw = entry_info(self.sa_d, self.dict, self.dinfo_plain)
        self.plcp_first, self.longs, self.plcp_irr = dict_irreducible(self.dict, self.sa_d, self.esuf, self.ebw)
        self.plcp = plcp_running_max(self.plcp_irr)
        self.lcp_gathered = self.plcp[self.sa_d]
        self.lcp_d = dict_lcp_clamp(self.lcp_gathered, self.esuf)
        self.gflag, self.pflag, self.vflag, self.seg = group_flags(self.esuf, self.lcp_d, w)
        self.segmin = segmin(self.seg)
        self.pscan, self.prank = phrase_ranks(self.esuf, self.ephr, self.pflag, D)
        self.parse = self.prank[self.pid]
        self.which, self.slen = invert_ranks(self.prank, self.rep, self.dlen)
        if not with_lists:
            return
        self.sa_p = K.ref_suffix_array(self.parse)
        self.sl = parse_sl(v, self.nv, self.sa_p, self.pstart)
        self.n_irreducible, self.n_long = parse_irreducible(v, self.nv, self.sa_p, self.pid, self.pstart)
        self.nb, self.levels, self.bmin = rmq_tables(self.sl)
        self.occ_keys, self.occ_vals = occ_sequence(self.sa_p, self.pid, D)
        o = np.argsort(self.occ_keys, kind="stable")
        self.occ_ids, self.occ_ts = self.occ_keys[o], self.occ_vals[o]
        self.pos_bits = 32
        self.occ_start, self.occ, self.occ_sl, self.occ12 = occ_lists(self.occ_ids, self.occ_ts, self.sa_p, self.pstart, self.sl,
                                                                      self.pos_bits, D + 1)
        self.tab = phrase_table(self.occ_start, self.plen, self.rep)
        self.gscan, self.vscan, self.ce = entry_compact(self.esuf, self.ephr, self.ebw, self.gflag, self.vflag, self.segmin, self.tab)
        self.E = len(self.ce["cnt"])
        self.ce_eoff = (np.cumsum(self.ce["cnt"].astype(np.int64)) - self.ce["cnt"]).astype(U32)
        self.sege = np.flatnonzero(self.ce["gs"]).astype(U32)
        self.G = len(self.sege)
        self.segb = np.concatenate([self.ce_eoff[self.sege], [n + 1]]).astype(U32)
        self.ghead = group_heads(self.sege, self.ce["hl"], self.ce["slen"])

    def dict_file(self):
        """the reference's .dict: the distinct phrases in lexicographic order, 0x01 behind each, 0x00 at the end"""
        out = []
        for ph in self.which:
            a, l = self.pstart[ph], self.plen[ph]
            out.append(self.v[a:a + l].tobytes() + b"\x01")
        return b"".join(out) + b"\x00"
