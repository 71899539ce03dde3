"""A CPU model of the launch wrappers of csrc/guided_kernels.hpp (mmt::gk, the bucket-wise producer): one function per
wrapper, named as the wrapper.  Plain Python and numpy, integers only, no tolerance; nothing is imported from the product.
tests/test_guided_model_host.py holds the model to independent statements (naive counts, sorted(), bisect), so that a broken
model cannot make a GPU test pass vacuously.

Conventions:
  * an in/out array goes in as the caller filled it (sentinels) and comes back with exactly the entries the wrapper writes
    changed: what the model leaves alone the kernel must leave alone;
  * where a kernel's output ORDER is not defined the model returns the canonical (sorted) form and says so in ORDER_FREE;
    the GPU tests may compare as sets there and nowhere else.
"""
import bisect

import numpy as np

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
M64 = (1 << 64) - 1
NO_BOUND = 0xFFFFFFFF
NONE64 = M64
TILE = 4096
SORT_CAP = 2048                 # elements of one LDS tile of local_sort
SHORT = 64                      # local_sort: a tile whose groups all have at most SHORT members is placed by counting (stable)
MEDIUM = 128
MEDIUM_BOUNDS = (16, 32, 64, 128)

# outputs whose order the kernels do not define (atomics hand out the slots): wrapper -> what is compared as a set
ORDER_FREE = {
    "medium_groups": "the (first, size) pairs inside each of the four regions of `list`",
    "range_groups": "the (begin, end) segments",
    "local_sort": "the (begin, end) pairs of big_*; and, in a tile sorted by the network (a group longer than SHORT), the "
                  "order of elements with equal (group, key)",
}


def _popcount(x):
    return bin(int(x)).count("1")


# ---- phrase ends ---------------------------------------------------------------------------------------------------------
def cut_mask(cuts, n_words):
    """bit c of the 64-bit words <=> a phrase ends at text position c"""
    words = [0] * n_words
    for c in cuts:
        words[int(c) >> 6] |= 1 << (int(c) & 63)
    return np.array(words, dtype=U64)


def cuts_of_mask(mask):
    return [64 * wi + b for wi, x in enumerate(mask) for b in range(64) if (int(x) >> b) & 1]


def mask_words(n):
    """whole blocks of 4096 positions, one block to spare behind the text's last (guided.cpp: n_blocks >= n / 4096 + 2)"""
    return (n // TILE + 2) * 64


def rank_counts(mask, n_counts, counts):
    """counts[j] = phrase ends at positions [512 j, 512 j + 512) (words past the end count nothing)"""
    cuts = cuts_of_mask(mask)
    out = counts.copy()
    for j in range(n_counts):
        out[j] = sum(1 for c in cuts if 512 * j <= c < 512 * (j + 1))
    return out


def block_first_cut(mask, n_blocks, first):
    """first[b] = the first phrase end of block b (4096 positions), 2^64 - 1 when it has none"""
    cuts = cuts_of_mask(mask)
    out = first.copy()
    for b in range(n_blocks):
        inside = [c for c in cuts if TILE * b <= c < TILE * (b + 1)]
        out[b] = inside[0] if inside else NONE64
    return out


def block_cut_counts(mask, n_blocks, counts):
    cuts = cuts_of_mask(mask)
    out = counts.copy()
    for b in range(n_blocks):
        out[b] = sum(1 for c in cuts if TILE * b <= c < TILE * (b + 1))
    return out


def block_cut_offsets(mask, brank, n_blocks, coff):
    """coff[brank[b] + i] = offset inside block b of its i-th phrase end"""
    cuts = cuts_of_mask(mask)
    out = coff.copy()
    for b in range(n_blocks):
        inside = [c - TILE * b for c in cuts if TILE * b <= c < TILE * (b + 1)]
        for i, o in enumerate(inside):
            out[int(brank[b]) + i] = o
    return out


class CutTables:
    """Both layouts of the phrase ends of a text of n characters with trigger window w, as guided.cpp derives them from the
    four wrappers above: bits (mask, rdir = ends before position 512 j) and list (coff, brank = ends before block b,
    blocks + 2 entries); nxt[b] = first end at or after 4096 b that lies below n, else n + w - 1."""

    def __init__(self, cuts, n, w):
        self.cuts = sorted(int(c) for c in cuts)
        assert all(0 <= c < n for c in self.cuts)
        self.n, self.w = n, w
        self.n_words = mask_words(n)
        self.n_blocks = self.n_words // 64
        self.mask = cut_mask(self.cuts, self.n_words)
        z32 = np.zeros
        rc = rank_counts(self.mask, self.n_words // 8, z32(self.n_words // 8, U32))
        self.rdir = np.concatenate([[0], np.cumsum(rc.astype(np.int64))[:-1]]).astype(U32)
        bc = block_cut_counts(self.mask, self.n_blocks, z32(self.n_blocks + 2, U32))
        self.brank = np.concatenate([[0], np.cumsum(bc.astype(np.int64))[:-1]]).astype(U32)
        self.coff = block_cut_offsets(self.mask, self.brank, self.n_blocks, z32(len(self.cuts) + 64, U16))
        first = block_first_cut(self.mask, self.n_blocks, z32(self.n_blocks, U64))
        nxt = [0] * (self.n_blocks + 1)
        nxt[self.n_blocks] = n + w - 1
        for b in range(self.n_blocks - 1, -1, -1):
            f = int(first[b])
            nxt[b] = nxt[b + 1] if f == NONE64 or f >= n else f
        self.nxt = np.array(nxt, dtype=U64)

    # the definition
    def next_cut(self, x):
        if x >= self.n:
            return self.n + self.w - 1
        k = bisect.bisect_left(self.cuts, x)
        return self.cuts[k] if k < len(self.cuts) else self.n + self.w - 1

    def rank1(self, x):
        return bisect.bisect_left(self.cuts, min(x, self.n))

    # the same answers read from the tables of one layout
    def next_cut_bits(self, x):
        if x >= self.n:
            return self.n + self.w - 1
        wi = x >> 6
        word = int(self.mask[wi]) & (M64 << (x & 63)) & M64
        stop = ((x >> 12) + 1) << 6
        while True:
            if word:
                return wi * 64 + (word & -word).bit_length() - 1
            wi += 1
            if wi == stop:
                return int(self.nxt[(x >> 12) + 1])
            word = int(self.mask[wi])

    def rank1_bits(self, x):
        x = min(x, self.n)
        r = int(self.rdir[x >> 9])
        for wi in range((x >> 9) << 3, x >> 6):
            r += _popcount(self.mask[wi])
        if x & 63:
            r += _popcount(int(self.mask[x >> 6]) & ((1 << (x & 63)) - 1))
        return r

    def _lower(self, b, t):
        lo, hi = int(self.brank[b]), int(self.brank[b + 1])
        return lo + bisect.bisect_left([int(v) for v in self.coff[lo:hi]], t), hi

    def next_cut_list(self, x):
        if x >= self.n:
            return self.n + self.w - 1
        b = x >> 12
        k, hi = self._lower(b, x & 4095)
        return (b << 12) + int(self.coff[k]) if k < hi else int(self.nxt[b + 1])

    def rank1_list(self, x):
        x = min(x, self.n)
        return self._lower(x >> 12, x & 4095)[0]


# ---- staged lists (the context-free half) ---------------------------------------------------------------------------------
def stage_block_tiles(tile_off, n_tiles, n, blk_tile):
    """blk_tile[B] = the LAST tile t with tile_off[t] <= 4096 B (the tile that holds entry 4096 B of a list of n entries;
    empty tiles share their offset with the tile behind them), blk_tile[blocks] = n_tiles - 1.  n = 0: nothing is written."""
    out = blk_tile.copy()
    if n == 0:
        return out
    blocks = (n + 4095) // 4096
    for b in range(blocks):
        out[b] = max(t for t in range(n_tiles) if t == 0 or int(tile_off[t]) <= 4096 * b)
    out[blocks] = n_tiles - 1
    return out


def stage_count(staged, b0, b1, block_count):
    """block_count[B] = entries of block B (4096 entries) whose bin (entry >> 12) lies in [b0, b1)"""
    out = block_count.copy()
    n = len(staged)
    for blk in range((n + 4095) // 4096):
        bins = np.asarray(staged[4096 * blk:4096 * (blk + 1)], dtype=np.int64) >> 12
        out[blk] = int(((bins >= b0) & (bins < b1)).sum())
    return out


# ---- first keys and rounds ------------------------------------------------------------------------------------------------
def key_symbols(key, bits, chars):
    """the `chars` symbol codes of a key, first symbol first"""
    return [(int(key) >> (bits * (chars - 1 - i))) & ((1 << bits) - 1) for i in range(chars)]


def common_symbols(a, b, bits, chars):
    n = 0
    for x, y in zip(key_symbols(a, bits, chars), key_symbols(b, bits, chars)):
        if x != y:
            break
        n += 1
    return n


def heads0(keys, bits, chars, head, active, lcp):
    """head[j] = 1 where a new key starts; active[j] = 1 inside groups of two or more; lcp[j] (optional) = the leading symbols
    the keys of j and j - 1 share, written only at heads j > 0"""
    B = len(keys)
    head, active = head.copy(), active.copy()
    lcp = None if lcp is None else lcp.copy()
    for j in range(B):
        h = j == 0 or int(keys[j]) != int(keys[j - 1])
        nh = j + 1 == B or int(keys[j + 1]) != int(keys[j])
        head[j] = 1 if h else 0
        active[j] = 0 if (h and nh) else 1
        if lcp is not None and j and h:
            lcp[j] = common_symbols(keys[j], keys[j - 1], bits, chars)
    return head, active, lcp


def gather_active(idx, pos_sorted, head, slot, pos, headval):
    slot, pos, headval = slot.copy(), pos.copy(), headval.copy()
    for c, j in enumerate(idx):
        slot[c] = j
        pos[c] = pos_sorted[j]
        headval[c] = c if head[j] else 0
    return slot, pos, headval


def groups_of(ghead):
    """[(first, size)] of a list of group heads (ghead[c] = index of the first element of c's group)"""
    out = []
    m = len(ghead)
    c = 0
    while c < m:
        d = c
        while d + 1 < m and int(ghead[d + 1]) == int(ghead[c]):
            d += 1
        assert int(ghead[c]) == c
        out.append((c, d - c + 1))
        c = d + 1
    return out


def medium_class(size):
    for cl, b in enumerate(MEDIUM_BOUNDS):
        if size <= b:
            return cl
    return None


def medium_groups(ghead):
    """(regions, count4): regions[cl] = the sorted (first, size) pairs of the groups of class cl -- EVERY group of at most 128
    elements is listed, the small ones included (the class of sizes <= 16); ORDER_FREE inside a region"""
    regions = [[], [], [], []]
    for first, size in groups_of(ghead):
        cl = medium_class(size)
        if cl is not None:
            regions[cl].append((first, size))
    return regions, [len(r) for r in regions]


def tile_bounds(ghead, target, limit, n_tiles, bound):
    """bound[0] = 0, bound[n_tiles] = m; bound[t] = the first group head in [t target, min(t target + limit, m)), m when that
    stretch reaches m (or begins there) without one, NO_BOUND otherwise"""
    m = len(ghead)
    out = bound.copy()
    heads = [c for c in range(m) if int(ghead[c]) == c]
    for t in range(n_tiles + 1):
        if t == 0:
            out[t] = 0
        elif t == n_tiles:
            out[t] = m
        else:
            c0 = t * target
            stop = min(c0 + limit, m)
            inside = [c for c in heads if c0 <= c < stop]
            out[t] = inside[0] if inside else (m if stop >= m else NO_BOUND)
    return out


def tile_ranges(bound):
    """[(begin, end)] of the non-empty tiles: from a bound to the next bound that is not NO_BOUND"""
    out = []
    n_tiles = len(bound) - 1
    for t in range(n_tiles):
        b = int(bound[t])
        if b == NO_BOUND:
            continue
        u = t + 1
        while int(bound[u]) == NO_BOUND:
            u += 1
        if int(bound[u]) > b:
            out.append((b, int(bound[u])))
    return out


def local_sort(kin, pin, ghead, bound, kout, pout, big_cap):
    """Every tile of at most SORT_CAP elements is sorted by (group, key): kout / pout at the tile's slots.  A tile whose groups
    all have at most SHORT members is sorted stably; one that holds a longer group goes through a network, which is not stable
    (ORDER_FREE).  A longer tile is listed (big, sorted here; the first big_cap pairs reach the lists, in any order, and the
    count counts them all) and its slots are NOT written.
    Returns (kout, pout, big, network) -- network = the (begin, end) of the tiles sorted by the network."""
    kout, pout = kout.copy(), pout.copy()
    big, network = [], []
    for b, e in tile_ranges(bound):
        if e - b > SORT_CAP:
            big.append((b, e))
            continue
        order = sorted(range(b, e), key=lambda i: (int(ghead[i]), int(kin[i]), i))
        for o, i in enumerate(order):
            kout[b + o] = kin[i]
            pout[b + o] = pin[i]
        sizes = {}
        for i in range(b, e):
            sizes[int(ghead[i])] = sizes.get(int(ghead[i]), 0) + 1
        if max(sizes.values()) > SHORT:
            network.append((b, e))
    return kout, pout, sorted(big), network


def range_groups(ghead, big_begin, big_end):
    """the (head, end) of every group that ENDS inside a listed range (a range ends its last group); ORDER_FREE"""
    out = []
    for b, e in zip(big_begin, big_end):
        for c in range(int(b), int(e)):
            if c + 1 == int(e) or int(ghead[c + 1]) == c + 1:
                out.append((int(ghead[c]), c + 1))
    return sorted(out)


def round_apply(pos_sorted, newhead, slot, out, flags):
    """an element that is a group of its own after the round leaves for out[slot]; flags = 1 for the others"""
    m = len(newhead)
    out, flags = out.copy(), flags.copy()
    for c in range(m):
        single = int(newhead[c]) == c and (c + 1 == m or int(newhead[c + 1]) == c + 1)
        if single:
            out[int(slot[c])] = pos_sorted[c]
        flags[c] = 0 if single else 1
    return out, flags


def round_compact(idx, slot, pos_sorted, newhead, slot_out, pos_out, headval_out):
    slot_out, pos_out, headval_out = slot_out.copy(), pos_out.copy(), headval_out.copy()
    for c, o in enumerate(idx):
        slot_out[c] = slot[o]
        pos_out[c] = pos_sorted[o]
        headval_out[c] = c if int(newhead[o]) == int(o) else 0
    return slot_out, pos_out, headval_out


# ---- giant bookkeeping -----------------------------------------------------------------------------------------------------
def flag_greater(v, thr, flags):
    out = flags.copy()
    out[:len(v)] = [1 if int(x) > thr else 0 for x in v]
    return out


def flag_spread(a, out):
    out = out.copy()
    n = len(a)
    for k in range(n):
        out[k] = int(a[k]) | (int(a[k - 1]) if k else 0) | (int(a[k + 1]) if k + 1 < n else 0)
    return out


def flag_to_distinct(occ_flag, pid, dflag):
    out = dflag.copy()
    for f, d in zip(occ_flag, pid):
        if f:
            out[d] = 1
    return out


def flag_from_distinct(dflag, pid, occ_flag):
    out = occ_flag.copy()
    for k, d in enumerate(pid):
        out[k] = dflag[d]
    return out


def flag_scatter_ones(ids, flags):
    out = flags.copy()
    for i in ids:
        out[i] = 1
    return out


def giant_distinct(gids, rep, dlen, which, glen):
    which, glen = which.copy(), glen.copy()
    for i, g in enumerate(gids):
        which[i] = rep[g]
        glen[i] = dlen[g]
    return which, glen


def giant_bits(flags, bits):
    """bit k % 32 of bits[k / 32] = flags[k] != 0; a word that holds no flag at all is not written"""
    out = bits.copy()
    m = len(flags)
    for wi in range((m + 31) // 32):
        out[wi] = sum(1 << t for t in range(32) if 32 * wi + t < m and int(flags[32 * wi + t]) != 0)
    return out


def popcount_words(bits, out):
    out = out.copy()
    for i, x in enumerate(bits):
        out[i] = _popcount(x)
    return out


def giant_map(gids, gstart, dmap):
    out = dmap.copy()
    for g, s in zip(gids, gstart):
        out[g] = s
    return out


def giant_occurrences(gk, pid, pstart, dmap, gps, gbase):
    gps, gbase = gps.copy(), gbase.copy()
    for j, k in enumerate(gk):
        gps[j] = int(pstart[k])
        gbase[j] = dmap[pid[k]]
    return gps, gbase


def giant_group_flags(esuf, lcp, flags):
    """entry r starts a new group unless it spells the string of entry r - 1: same length (esuf without its top bit) and an LCP
    of at least that length"""
    out = flags.copy()
    for r in range(len(esuf)):
        sl = int(esuf[r]) & 0x7FFFFFFF
        out[r] = 1 if r == 0 or (int(esuf[r - 1]) & 0x7FFFFFFF) != sl or int(lcp[r]) < sl else 0
    return out


# ---- results (the context-free half) -----------------------------------------------------------------------------------------
def group_ids(ce_gs, gscan, B):
    out = ce_gs.copy()
    for e in range(B):
        out[e] = gscan[e] if int(ce_gs[e]) else 0
    return out


def add_offset(table, n, add):
    """table[i] += add in the table's own width (32 bits wrap)"""
    out = table.copy()
    mod = 1 << (8 * table.itemsize)
    for i in range(n):
        out[i] = (int(table[i]) + add) % mod
    return out


def rep_bits(pid, rep, bits):
    """bit k <=> rep[pid[k]] == k"""
    out = bits.copy()
    m = len(pid)
    for wi in range((m + 31) // 32):
        out[wi] = sum(1 << b for b in range(32) if 32 * wi + b < m and int(rep[pid[32 * wi + b]]) == 32 * wi + b)
    return out


# ==== the context (gk::Ctx) and the wrappers that read it ========================================================================
POS_MASK = (1 << 40) - 1
LEN_SAT = 0xFFFFFF
RANK_KEY = 1 << 63
GIANT_KEY = 1 << 62
LCP_CAP = 0xFFF00000
RUN_BUCKETS_HALF = 8448
NO_ENTRY = 0xFFFFFFFF
DOLLAR = 2


def code_table(text):
    """symbol codes ascending with the byte value, from 1; the Dollar always has one; 0 = a byte that does not occur.
    (code, bits per code, characters per 63-bit key)"""
    present = set(int(b) for b in text) | {DOLLAR}
    code = np.zeros(256, U8)
    for i, b in enumerate(sorted(present)):
        code[b] = i + 1
    bits = max(1, len(present).bit_length())
    return code, bits, min(63 // bits, 63)


class Ctx:
    """What the kernels know about a text: V = Dollar . T . Dollar^32 . zeros (V index q = text position + 1), the phrase ends
    (`cuts`, text positions, any ascending list below n: a forged parse is as good as a real one), the symbol codes, and how an
    element record is laid out.  Optional: isa_p (rank of the parse suffix that starts at phrase k), pid, repbits (one bit per
    phrase: 1 = keep its suffixes), giant (see Giant)."""

    def __init__(self, text, w, cuts, code=None, bits=None, chars=None, skip=0, pos_bits=40, rec_rank=0, isa_p=None, pid=None,
                 rep=None, expand=0, giant=None, g_depth=0):
        self.text = np.asarray(text, dtype=U8)
        self.n, self.w = len(self.text), w
        self.t = CutTables(cuts, self.n, w)
        self.cuts = self.t.cuts
        self.m = len(self.cuts) + 1
        if code is None:
            code, bits, chars = code_table(self.text)
        self.code, self.bits, self.chars = np.asarray(code, dtype=U8), bits, chars
        self.skip, self.pos_bits, self.rec_rank, self.expand = skip, pos_bits, rec_rank, expand
        self.isa_p = None if isa_p is None else np.asarray(isa_p, dtype=U32)
        self.pid = None if pid is None else np.asarray(pid, dtype=U32)
        self.rep = None if rep is None else [int(x) for x in rep]           # rep[k] = 1: phrase k is a representative occurrence
        self.giant, self.g_depth = giant, g_depth
        self.tiles = max(1, (self.n + TILE - 1) // TILE)
        # vs[q] = symbol code of V[q], far enough behind the text for every window a kernel stages (the same values as sym())
        v = np.zeros((self.tiles + 1) * TILE + 256, U8)
        v[0] = DOLLAR
        v[1:self.n + 1] = self.text
        v[self.n + 1:self.n + 33] = DOLLAR
        self.vs = self.code[v].astype(np.int64)
        self._bins, self._runs, self._all = {}, {}, None

    def bins(self, pc):
        """bin of every text position (the first pc symbols of its suffix), as one array"""
        if pc not in self._bins:
            b = np.zeros(self.tiles * TILE, np.int64)
            for i in range(pc):
                b = (b << self.bits) | self.vs[1 + i:1 + i + len(b)]
            self._bins[pc] = b
        return self._bins[pc]

    def all_suffixes(self):
        """(keys, records, keep) of every text position at once -- the same values as pack_chars, make_rec and keep give one
        by one (tests/test_guided_model_host.py compares them), for the models that walk whole texts"""
        if self._all is None:
            n = self.n
            q = np.arange(1, n + 1, dtype=np.int64)
            keys = np.zeros(n, U64)
            for i in range(self.chars):
                keys = (keys << U64(self.bits)) | self.vs[1 + i:1 + i + n].astype(U64)
            cuts = np.array(self.cuts, dtype=np.int64)
            x = q + self.skip + self.w - 2
            at = np.searchsorted(cuts, x, "left")
            end = np.where((at < len(cuts)) & (x < n), cuts[np.minimum(at, max(len(cuts) - 1, 0))] if len(cuts) else 0, n + self.w - 1)
            if self.rec_rank:
                k = np.searchsorted(cuts, np.minimum(x, n), "left")
                after = np.where(k + 1 < self.m, self.isa_p.astype(np.int64)[np.minimum(k + 1, self.m - 1)], 0)
                recs = q.astype(U64) | (after.astype(U64) << U64(self.pos_bits))
            else:
                recs = q.astype(U64) | (np.minimum(end + 2 - q, LEN_SAT).astype(U64) << U64(40))
            if self.rep is None:
                keep = np.ones(n, bool)
            else:
                keep = np.array(self.rep, dtype=bool)[np.searchsorted(cuts, np.minimum(q - 1 + self.w - 1, n), "left")]
            self._all = (keys, recs, keep)
        return self._all

    def tile_runs(self, sym):
        """rl[p] = length of the run of `sym` that begins at text position p, counted up to the end of p's tile"""
        if sym not in self._runs:
            total = self.tiles * TILE
            rl = np.zeros(total + 1, np.int64)
            for p in range(total - 1, -1, -1):
                if self.vs[p + 1] == sym:
                    rl[p] = 1 + (rl[p + 1] if (p + 1) % TILE else 0)
            self._runs[sym] = rl
        return self._runs[sym]

    # -- the text
    def vbyte(self, q):
        if q == 0:
            return DOLLAR
        p = q - 1
        return int(self.text[p]) if p < self.n else (DOLLAR if p < self.n + 32 else 0)

    def sym(self, p):
        """symbol code at text position p (the Dollars behind the text have theirs, the zeros behind those have 0)"""
        return int(self.code[self.vbyte(p + 1)])

    def pack_chars(self, q):
        key = 0
        for i in range(self.chars):
            key = (key << self.bits) | int(self.code[self.vbyte(q + i)])
        return key

    def bin_of(self, p, pc):
        b = 0
        for i in range(pc):
            b = (b << self.bits) | self.sym(p + i)
        return b

    def phrase_start(self, k):
        """V index of the first character of phrase k"""
        return 0 if k == 0 else self.cuts[k - 1] - self.w + 2

    def phrase_len(self, k):
        return (self.cuts[k] + 1 if k < len(self.cuts) else self.n + self.w) - self.phrase_start(k) + 1

    # -- phrase ends and records
    def query_point(self, q):
        return q + self.skip + self.w - 2

    def phrase_of(self, q):
        return self.t.rank1(self.query_point(q))

    def alpha_len(self, q):
        return self.t.next_cut(self.query_point(q)) + 2 - q

    def rank_after(self, q):
        """rank of the parse suffix that follows the element's phrase (0: the last phrase)"""
        k = self.phrase_of(q)
        return int(self.isa_p[k + 1]) if k + 1 < self.m else 0

    def make_rec(self, q):
        if self.rec_rank:
            return q | (self.rank_after(q) << self.pos_bits)
        return q | (min(self.alpha_len(q), LEN_SAT) << 40)

    def rec_pos(self, rec):
        return int(rec) & ((1 << self.pos_bits) - 1)

    def rec_len(self, rec):
        """the length of alpha whatever the record's form (a saturated or forged LEN_SAT is looked up again)"""
        q = self.rec_pos(rec)
        if self.rec_rank or (int(rec) >> 40) == LEN_SAT:
            return self.alpha_len(q)
        return int(rec) >> 40

    def rec_rank_key(self, rec):
        q = self.rec_pos(rec)
        if self.expand:
            return q
        if self.rec_rank:
            return int(rec) >> self.pos_bits
        return self.rank_after(q)

    def keep(self, p):
        """expansion: the suffix at text position p starts in a representative occurrence (no table: every suffix)"""
        return True if self.rep is None else bool(self.rep[self.t.rank1(p + self.w - 1)])

    def bitwords(self, flags):
        words = [0] * (self.m // 32 + 1)
        for k, f in enumerate(flags):
            if f:
                words[k >> 5] |= 1 << (k & 31)
        return np.array(words, dtype=U32)

    def giant_entry(self, q, off):
        """the entry of the giant dictionary's suffix array for the element at V index q, `off` characters in; None when its
        phrase is not a giant occurrence"""
        g = self.giant
        if g is None:
            return None
        k = self.phrase_of(q)
        if not g.flag[k]:
            return None
        lo = sum(g.flag[:k])
        return int(g.isa[int(g.base[lo]) + (q + off - int(g.ps[lo]))])


class Giant:
    """The giant tables as the kernels read them: flag[k] = phrase k is a giant occurrence; for the j-th of them g_k[j] = k,
    g_ps[j] = the V index of its first character, g_base[j] = where its phrase lies in the giant dictionary; g_isa[position] =
    entry of the dictionary's suffix array, g_grp[entry] = its group of equal strings, lcp[entry] = the dictionary's LCP array.
    (Lookups only: the kernels never read the dictionary itself, so any tables of the right shape are legal inputs.)"""

    def __init__(self, ctx_flags, starts, base, isa, grp, lcp):
        self.flag = [int(f) for f in ctx_flags]
        self.k = np.array([k for k, f in enumerate(self.flag) if f], dtype=U32)
        self.ps = np.array([starts[k] for k in self.k], dtype=U64)
        self.base = np.asarray(base, dtype=U32)
        self.isa, self.grp, self.lcp = np.asarray(isa, dtype=U32), np.asarray(grp, dtype=U32), np.asarray(lcp, dtype=U32)
        assert len(self.base) == len(self.k) and len(self.grp) == len(self.isa) == len(self.lcp)

    def rank_words(self, bits):
        """giant occurrences before phrase 32 j"""
        out, acc = [], 0
        for x in bits:
            out.append(acc)
            acc += _popcount(x)
        return np.array(out, dtype=U32)


class RunSlice:
    """gk::RunSlice: the suffixes c^r X of the bin of the repeated symbol `sym` whose bucket lies in [blo, bhi); per tile: the
    symbol at its first position, the length of the run of it that begins there (may span many tiles: a table the host chains,
    so any value is a legal input) and the symbol behind that run."""

    def __init__(self, sym, blo, bhi, lead, first, follow):
        self.sym, self.blo, self.bhi = sym, blo, bhi
        self.lead, self.first, self.follow = np.asarray(lead, dtype=U64), np.asarray(first, dtype=U8), np.asarray(follow, dtype=U8)
        self.n_tiles = len(self.lead)


def run_f(r):
    if r < 256:
        return r
    e = r.bit_length() - 1
    return (e - 7) * 256 + ((r >> (e - 8)) & 0xFF)


def run_bucket(r, below):
    """bucket of K = (X0 < c ? r : 2^41 - r): r exact below 256, then 256 buckets per power of two, r capped at 2^40 - 1"""
    f = run_f(min(r, (1 << 40) - 1))
    return f if below else 2 * RUN_BUCKETS_HALF - 1 - f


def run_at(c, rs, p):
    """(r, bucket) of the suffix at text position p: r = length of the run of rs.sym that begins there -- counted inside p's
    tile, and continued by the table entry of the next tile when it reaches the tile's end (no entry: nothing follows, and the
    symbol behind the run reads 0)"""
    tile = p // TILE
    end = (tile + 1) * TILE
    r = int(c.tile_runs(rs.sym)[p])
    x = p + r
    if x < end:
        follow = c.sym(x)
    else:
        follow = 0
        if tile + 1 < rs.n_tiles:
            if int(rs.first[tile + 1]) == rs.sym:
                r += int(rs.lead[tile + 1])
                follow = int(rs.follow[tile + 1])
            else:
                follow = int(rs.first[tile + 1])
    return r, (run_bucket(r, follow < rs.sym) if r else 0)


def in_slice(c, rs, p):
    if rs is None:
        return True
    r, b = run_at(c, rs, p)
    return r > 0 and rs.blo <= b < rs.bhi


def dense_tiles(c, text_layout, no_dense=False):
    """the tiles the text-order kernels read as 2-bit words: a packed text, codes for all four bases, at most 32 characters a
    key, 64 characters of text behind the tile, and no exception (anything but A C G T) in the tile's block of 4096 positions
    or in the next -- a property of the input, from which the tests count which path a launch takes"""
    ok = text_layout == "packed" and not no_dense and c.chars <= 32 and all(int(c.code[b]) for b in b"ACGT")
    exc = ~np.isin(c.text, np.frombuffer(b"ACGT", U8))
    flagged = set((np.flatnonzero(exc) // TILE).tolist())
    return [t for t in range(c.tiles) if ok and t * TILE + TILE + 64 <= c.n and t not in flagged and t + 1 not in flagged]


def codes64_readable(c, q):
    """a packed text hands out V[q .. q + 64) as two words of 2-bit codes only when all of them are text and neither block of
    4096 positions they touch holds an exception (textref.hpp: one flag per block); else the reader falls back to bytes"""
    if q < 1 or q + 63 > c.n:
        return False
    flagged = set((np.flatnonzero(~np.isin(c.text, np.frombuffer(b"ACGT", U8))) // TILE).tolist())
    return (q - 1) // TILE not in flagged and (q + 62) // TILE not in flagged


def tile_lead(c, first, lead, follow):
    first, lead, follow = first.copy(), lead.copy(), follow.copy()
    for t in range(c.tiles):
        s0 = c.sym(t * TILE)
        k = 0
        while k < TILE and c.sym(t * TILE + k) == s0:
            k += 1
        first[t], lead[t], follow[t] = s0, k, (c.sym(t * TILE + k) if k < TILE else 0)
    return first, lead, follow


def chain_leads(first, lead, follow, n_tiles):
    """the host's chain over tile_lead's tables: the whole length of the run that begins at a tile's first position"""
    out = [0] * n_tiles
    fol = [0] * n_tiles
    for t in range(n_tiles - 1, -1, -1):
        out[t], fol[t] = int(lead[t]), int(follow[t])
        if int(lead[t]) == TILE:
            if t + 1 < n_tiles and int(first[t + 1]) == int(first[t]):
                out[t] += out[t + 1]
                fol[t] = fol[t + 1]
            elif t + 1 < n_tiles:
                fol[t] = int(first[t + 1])
    return np.array(out, dtype=U64), np.array(fol, dtype=U8)


def selected(c, pc, lo, hi, rs=None):
    """text positions of the suffixes of bins [lo, hi) that the expansion keeps and the slice holds, ascending"""
    b = c.bins(pc)[:c.n]
    return [int(p) for p in np.flatnonzero((b >= lo) & (b < hi) & c.all_suffixes()[2]) if in_slice(c, rs, int(p))]


def bin_hist(c, pc, hist):
    out = hist.copy()
    b = c.bins(pc)[:c.n][c.all_suffixes()[2]]
    out[:1 << (c.bits * pc)] += np.bincount(b, minlength=1 << (c.bits * pc)).astype(U64)
    return out


def batch_count(c, pc, lo, hi, tile_count, rs=None):
    out = tile_count.copy()
    sel = np.array(selected(c, pc, lo, hi, rs), dtype=np.int64)
    out[:c.tiles] = np.bincount(sel // TILE, minlength=c.tiles).astype(U32)
    return out


def run_hist(c, pc, bin_, rs, hist):
    """hist[b] = suffixes of the run bin in bucket b, hist[2 HALF + b] = those the expansion keeps (all buckets: the slice's
    range is not looked at)"""
    out = hist.copy()
    for p in np.flatnonzero(c.bins(pc)[:c.n] == bin_):
        p = int(p)
        r, b = run_at(c, rs, p)
        if r:
            out[b] += U64(1)
            if c.keep(p):
                out[2 * RUN_BUCKETS_HALF + b] += U64(1)
    return out


def batch_fill(c, pc, lo, hi, tile_off, keys, pos, next_lo, next_hi, next_count, rs=None):
    """the selected suffixes of every tile, in text order, from the tile's offset on: first key and element record;
    next_count (optional) = per tile the kept suffixes of bins [next_lo, next_hi) -- whatever the slice"""
    keys, pos = keys.copy(), pos.copy()
    at = [int(x) for x in tile_off[:c.tiles]]
    all_keys, all_recs, _ = c.all_suffixes()
    for p in selected(c, pc, lo, hi, rs):
        t = p // TILE
        keys[at[t]] = all_keys[p]
        pos[at[t]] = all_recs[p]
        at[t] += 1
    if next_count is not None:
        next_count = batch_count(c, pc, next_lo, next_hi, next_count)
    return keys, pos, next_count


def stage_fill(c, pc, lo, hi, tile_off, staged, next_lo, next_hi, next_count):
    staged = staged.copy()
    at = [int(x) for x in tile_off[:c.tiles]]
    b = c.bins(pc)
    for p in selected(c, pc, lo, hi):
        t = p // TILE
        staged[at[t]] = (p & 4095) | (int(b[p]) << 12)
        at[t] += 1
    if next_count is not None:
        next_count = batch_count(c, pc, next_lo, next_hi, next_count)
    return staged, next_count


def stage_take(c, staged, b0, b1, block_off, keys, pos, nb0, nb1, next_count, tile_off):
    """what a batch -- bins [b0, b1) -- takes from a staged list: per block of 4096 entries, in list order, from the block's
    offset on; the tile of entry i is the last tile whose offset is at most i"""
    keys, pos = keys.copy(), pos.copy()
    next_count = None if next_count is None else next_count.copy()
    n = len(staged)
    offs = [int(x) for x in tile_off[:c.tiles]]
    all_keys, all_recs, _ = c.all_suffixes()
    for blk in range((n + 4095) // 4096):
        at = int(block_off[blk])
        nxt = 0
        for i in range(4096 * blk, min(n, 4096 * (blk + 1))):
            e = int(staged[i])
            if nb0 <= (e >> 12) < nb1:
                nxt += 1
            if b0 <= (e >> 12) < b1:
                tile = bisect.bisect_right(offs, i) - 1
                p = tile * TILE + (e & 4095)
                keys[at] = all_keys[p] if p < c.n else c.pack_chars(p + 1)
                pos[at] = all_recs[p] if p < c.n else c.make_rec(p + 1)
                at += 1
        if next_count is not None:
            next_count[blk] = nxt
    return keys, pos, next_count


def phrase_items(c, pstart, rep, keys, pos):
    keys, pos = keys.copy(), pos.copy()
    for d, k in enumerate(rep):
        q = int(pstart[k])
        keys[d] = c.pack_chars(q)
        pos[d] = c.make_rec(q)
    return keys, pos


def giant_probe(c, pos, ghead, offset, gr, pure):
    """gr[e] = the element's entry at `offset` (NO_ENTRY: alpha is spent there, or the phrase is no giant occurrence);
    pure[first member] = 1 when every member of the group has one (all m bytes are set: 1 unless cleared)"""
    gr, pure = gr.copy(), pure.copy()
    m = len(pos)
    pure[:m] = 1
    for e in range(m):
        r = None if offset >= c.rec_len(pos[e]) else c.giant_entry(c.rec_pos(pos[e]), offset)
        gr[e] = NO_ENTRY if r is None else r
        if r is None:
            pure[int(ghead[e])] = 0
    return gr, pure


def round_keys(c, pos, offset, keys, err, gr=None, pure=None, ghead=None):
    """the key of a round: a pure group's entries; alpha spent -> the rank that follows (phrases: err[0], the element's index);
    beyond g_depth inside a giant occurrence -> the entry; else the next `chars` symbols"""
    keys, err = keys.copy(), err.copy()
    for e in range(len(pos)):
        if gr is not None and pure[int(ghead[e])]:
            keys[e] = GIANT_KEY | int(gr[e])
            continue
        q = c.rec_pos(pos[e])
        if offset >= c.rec_len(pos[e]):
            if c.skip:
                err[0] += U32(1)
                keys[e] = RANK_KEY | e
            else:
                keys[e] = RANK_KEY | c.rec_rank_key(pos[e])
            continue
        r = c.giant_entry(q, offset) if c.giant is not None and offset >= c.g_depth else None
        keys[e] = c.pack_chars(q + offset) if r is None else (GIANT_KEY | r)
    return keys, err


def round_heads(c, keys, ghead, headval, err, lcp_out=None, slot=None, offset=0, pure=None):
    """headval[e] = e where a new group starts after the round's sort, else 0.  Inside an old group: a rank key always starts
    one (ranks are distinct); two giant entries -- only in a round beyond g_depth or in a pure group -- part when their groups
    of equal strings differ (and always under `expand`); characters part when the keys differ.  err[1] counts neighbours of one
    group of which one is spent and the other is not.  lcp_out[slot[e]]: written where two entries of different groups part
    (offset + the minimum of the dictionary's LCP array between them) and where two character keys part (offset + the symbols
    they share) -- nowhere else."""
    headval, err = headval.copy(), err.copy()
    lcp_out = None if lcp_out is None else lcp_out.copy()
    giant_round = c.giant is not None and offset >= c.g_depth
    for e in range(len(keys)):
        k, g0 = int(keys[e]), int(ghead[e])
        h = g0 == e
        if not h:
            kp = int(keys[e - 1])
            if (k >> 63) != (kp >> 63):
                err[1] += U32(1)
            h = (k >> 63) != 0 or k != kp
            as_entries = giant_round or (pure is not None and pure[g0])
            if as_entries and (k >> 32) == (GIANT_KEY >> 32) and (kp >> 32) == (GIANT_KEY >> 32):
                r, rp = k & 0xFFFFFFFF, kp & 0xFFFFFFFF
                differ = int(c.giant.grp[r]) != int(c.giant.grp[rp])
                h = differ or bool(c.expand)
                if differ and lcp_out is not None:
                    lcp_out[int(slot[e])] = min(offset + min(int(x) for x in c.giant.lcp[rp + 1:r + 1]), LCP_CAP)
            elif lcp_out is not None and k != kp and not ((k | kp) >> 63) and not as_entries:
                lcp_out[int(slot[e])] = min(offset + common_symbols(k, kp, c.bits, c.chars), LCP_CAP)
        headval[e] = e if h else 0
    return headval, err, lcp_out


def write_columns(c, pos, base, sa_lo, sa_hi, bwt):
    """SA entry = text position (32 bits, or 32 + 8), BWT = the character before it (0 before text position 0)"""
    sa_lo, bwt = sa_lo.copy(), bwt.copy()
    sa_hi = None if sa_hi is None else sa_hi.copy()
    for j, rec in enumerate(pos):
        q = c.rec_pos(rec)
        sa_lo[base + j] = (q - 1) & 0xFFFFFFFF
        if sa_hi is not None:
            sa_hi[base + j] = ((q - 1) >> 32) & 0xFF
        bwt[base + j] = 0 if q == 1 else c.vbyte(q - 1)
    return sa_lo, sa_hi, bwt


def phrase_ranks(c, pos, pid, prank):
    out = prank.copy()
    for j, rec in enumerate(pos):
        out[int(pid[c.phrase_of(c.rec_pos(rec))])] = j + 1
    return out


def expand_entries(c, pos, lcp, tab, cols, err):
    """cols: dict of the seven columns (cnt, first, offm1, bwt, gs, hl, slen).  err[1] counts elements whose alpha is not a
    proper suffix of at least w characters of its phrase."""
    cols = {k: v.copy() for k, v in cols.items()}
    err = err.copy()
    for e, rec in enumerate(pos):
        q = c.rec_pos(rec)
        slen = c.rec_len(rec)
        t = [int(x) for x in tab[int(c.pid[c.phrase_of(q)])]]
        if slen >= t[2] or slen < c.w:
            err[1] += U32(1)
        cols["cnt"][e], cols["first"][e] = t[0], t[1]
        cols["offm1"][e] = (t[2] - slen - 1) & 0xFFFFFFFF
        cols["bwt"][e] = 0 if q == 1 else c.vbyte(q - 1)
        cols["gs"][e] = 1 if e == 0 or int(lcp[e]) < slen else 0
        cols["hl"][e] = lcp[e]
        cols["slen"][e] = slen & 0xFFFFFFFF
    return cols, err


# ---- comparisons of phrase suffixes (no giant dictionary: the plain definition) ---------------------------------------------------
def alpha_cmp(c, qa, la, qb, lb):
    """(order, shared): the bytes of V behind qa and qb compared one by one up to the shorter alpha; order = -1 / +1 where a
    byte decides (shared = the characters before it), 0 when none does (shared = the shorter length): phrase suffixes are
    prefix-free, so the two spell the same alpha then"""
    L = min(la, lb)
    for t in range(L):
        x, y = c.vbyte(qa + t), c.vbyte(qb + t)
        if x != y:
            return (-1 if x < y else 1), t
    return 0, L


def resolve_small(c, pos, ghead, slot, offset, out, flags, err, lcp_out=None, limit=0):
    """Groups of at most `limit` (0: eight) members are finished: out[slot of the group's first + i] = the i-th member in the
    order (alpha; the same alpha: the rank that follows -- phrases: no order but the index, and err[0]; ties: the index),
    flags = 0.  Larger groups: flags = 1, nothing else.  err[1]: members that agree up to the shorter alpha but differ in its
    length (both of a pair count: 2).  lcp_out[slot + i], i >= 1: the LCP of the member with the one before it where a
    character parts them; the same alpha: |alpha| under `expand`, else untouched."""
    import functools
    out, flags, err = out.copy(), flags.copy(), err.copy()
    lcp_out = None if lcp_out is None else lcp_out.copy()
    lim = limit or 8
    for g0, size in groups_of(ghead):
        members = list(range(g0, g0 + size))
        if size > lim:
            flags[g0:g0 + size] = 1
            continue
        q = {e: c.rec_pos(pos[e]) for e in members}
        ln = {e: c.rec_len(pos[e]) for e in members}

        def order(a, b):
            s, _ = alpha_cmp(c, q[a], ln[a], q[b], ln[b])
            if s:
                return s
            if not c.skip:
                ka, kb = c.rec_rank_key(pos[a]), c.rec_rank_key(pos[b])
                if ka != kb:
                    return -1 if ka < kb else 1
            return -1 if a < b else 1
        for i, a in enumerate(members):
            for b in members[i + 1:]:
                if alpha_cmp(c, q[a], ln[a], q[b], ln[b])[0] == 0:
                    if c.skip:
                        err[0] += U32(2)
                    elif ln[a] != ln[b]:
                        err[1] += U32(2)
        ranked = sorted(members, key=functools.cmp_to_key(order))
        base = int(slot[g0])
        for i, e in enumerate(ranked):
            out[base + i] = pos[e]
            flags[e] = 0
            if lcp_out is not None and i:
                p = ranked[i - 1]
                s, t = alpha_cmp(c, q[p], ln[p], q[e], ln[e])
                if s:
                    lcp_out[base + i] = min(t, LCP_CAP)
                elif c.expand:
                    lcp_out[base + i] = min(ln[e], LCP_CAP)
    return out, flags, err, lcp_out


def batch_lcp(c, sl, pos, carry, lcp, err):
    """lcp[j] of a sorted batch: entries that are not 0xffffffff are kept (hints of the sort); lcp[0] = 0 without a carry; a
    pair that a character parts: the characters before it; the same alpha: |alpha| - w + the minimum of the parse's LCP array
    between the two ranks (under `expand`: |alpha|).  err[2]: the same alpha with different lengths, or ranks out of order."""
    lcp, err = lcp.copy(), err.copy()
    for j in range(len(pos)):
        if j == 0 and carry is None:
            lcp[0] = 0
            continue
        if int(lcp[j]) != 0xFFFFFFFF:
            continue
        ra, rb = pos[j], (pos[j - 1] if j else carry[0])
        la, lb = c.rec_len(ra), c.rec_len(rb)
        s, v = alpha_cmp(c, c.rec_pos(ra), la, c.rec_pos(rb), lb)
        if s == 0:
            if c.expand:
                if la != lb:
                    err[2] += U32(1)
            else:
                ka, kb = c.rec_rank_key(ra), c.rec_rank_key(rb)
                if la != lb or kb >= ka:
                    err[2] += U32(1)
                else:
                    v = la - c.w + min(int(x) for x in sl[kb + 1:ka + 1])
        lcp[j] = min(v, LCP_CAP)
    return lcp, err


MEDIUM_PER_WAVE = (4, 2, 1, 1)          # groups a wave of resolve_medium takes, by size class


def resolve_medium(c, sl, pos, slot, classes, offset, out, flags, err, lcp_out=None):
    """classes: for each of the four size classes the listed (first, size) groups, in list order.  EVERY listed group is
    finished (the kernel leaves none to the rounds): out[slot of its first + i] = its i-th member in resolve_small's order,
    flags = 0 for its members.  lcp_out[slot + i], i >= 1: the LCP of the member with the one before it -- the characters
    before the one that parts them; the same alpha: |alpha| - w + the minimum of the parse's LCP array between the two ranks
    (|alpha| alone under `expand`, or when the ranks do not ascend).  err[1] (phrases: err[0]) grows by ONE per wave -- 4 / 2 /
    1 / 1 consecutive groups of a class -- that holds two members which agree up to the shorter alpha and differ in its
    length (phrases: any two equal ones)."""
    import functools
    out, flags, err = out.copy(), flags.copy(), err.copy()
    lcp_out = None if lcp_out is None else lcp_out.copy()
    for cl, groups in enumerate(classes):
        bad_waves = set()
        for gi, (g0, size) in enumerate(groups):
            members = list(range(g0, g0 + size))
            q = {e: c.rec_pos(pos[e]) for e in members}
            ln = {e: c.rec_len(pos[e]) for e in members}
            key = {e: bytes(c.vbyte(q[e] + t) for t in range(ln[e])) for e in members}

            def order(a, b):
                if key[a] != key[b] and not (key[a].startswith(key[b]) or key[b].startswith(key[a])):
                    return -1 if key[a] < key[b] else 1
                if not c.skip:
                    ka, kb = c.rec_rank_key(pos[a]), c.rec_rank_key(pos[b])
                    if ka != kb:
                        return -1 if ka < kb else 1
                return -1 if a < b else 1
            ranked = sorted(members, key=functools.cmp_to_key(order))
            base = int(slot[g0])
            for i, e in enumerate(ranked):
                out[base + i] = pos[e]
                flags[g0 + i] = 0
                if i:
                    p = ranked[i - 1]
                    s, t = alpha_cmp(c, q[p], ln[p], q[e], ln[e])
                    if s == 0 and (ln[p] != ln[e] or c.skip):
                        bad_waves.add(gi // MEDIUM_PER_WAVE[cl])
                    if lcp_out is not None:
                        if s == 0:
                            ra, rb = (0, 0) if c.skip else (c.rec_rank_key(pos[p]), c.rec_rank_key(pos[e]))
                            t = ln[e] if c.expand or rb <= ra else ln[e] - c.w + min(int(x) for x in sl[ra + 1:rb + 1])
                        lcp_out[base + i] = min(t, LCP_CAP)
        err[0 if c.skip else 1] += U32(len(bad_waves))
    return out, flags, err, lcp_out


def medium_levels(c, recs, majority):
    """how deep the comparisons of a group's members go, from the input alone: (second, third) = pairs of members that differ
    from the majority's alpha at the same place with the same character, and those of them that agree beyond it up to a second
    shared difference with that first member's alpha"""
    qm, lm = c.rec_pos(recs[majority]), c.rec_len(recs[majority])
    first = {}
    for e, r in enumerate(recs):
        s, t = alpha_cmp(c, c.rec_pos(r), c.rec_len(r), qm, lm)
        if s:
            first.setdefault((t, c.vbyte(c.rec_pos(r) + t)), []).append(e)
    second = third = 0
    for kind in first.values():
        lead = kind[0]
        nxt = {}
        for e in kind[1:]:
            second += 1
            s, t = alpha_cmp(c, c.rec_pos(recs[e]), c.rec_len(recs[e]), c.rec_pos(recs[lead]), c.rec_len(recs[lead]))
            if s:
                nxt.setdefault((t, c.vbyte(c.rec_pos(recs[e]) + t)), []).append(e)
        third += sum(len(v) - 1 for v in nxt.values())
    return second, third


# ---- the giant dictionary, derived from the parse ---------------------------------------------------------------------------------
def derive_giant(c, keep=None):
    """The giant tables of a context from its own phrases: the distinct phrases longer than g_depth (keep(k), optional: which of
    the long occurrences are taken) laid one behind the other; the suffixes of every phrase -- each ends with its phrase --
    sorted naively (a proper prefix first); g_isa[position] = place of that suffix, g_grp = id of its run of equal strings,
    lcp[r] = characters entries r - 1 and r share.  Phrase suffixes of w characters and more are prefix-free, so for any two
    of them the order of their entries is the order of the alphas and the minimum of lcp between them is what they share."""
    flags = [1 if c.phrase_len(k) > c.g_depth and (keep is None or keep(k)) else 0 for k in range(c.m)]
    spelled, where, strings = {}, {}, []
    for k in range(c.m):
        if flags[k]:
            a = c.phrase_start(k)
            s = bytes(c.vbyte(a + t) for t in range(c.phrase_len(k)))
            if s not in spelled:
                spelled[s] = sum(len(x) for x in strings)
                strings.append(s)
            where[k] = spelled[s]
    sufs = []
    at = 0
    for s in strings:
        sufs += [(s[o:], at + o) for o in range(len(s))]
        at += len(s)
    sufs.sort()
    size = max(at, 1)
    isa, grp, lcp = np.zeros(size, U32), np.zeros(size, U32), np.zeros(size, U32)
    for r, (s, p) in enumerate(sufs):
        isa[p] = r
        if r:
            prev = sufs[r - 1][0]
            t = 0
            while t < min(len(s), len(prev)) and s[t] == prev[t]:
                t += 1
            lcp[r] = t
            grp[r] = grp[r - 1] + (0 if s == prev else 1)
    return Giant(flags, [c.phrase_start(k) for k in range(c.m)], [where[k] for k in range(c.m) if flags[k]], isa, grp, lcp)


# ---- a whole batch: the model's steps chained in the order guided.cpp chains the wrappers (sort_batch) ---------------------------
def _select(flags, m):
    return np.flatnonzero(np.asarray(flags[:m]) != 0).astype(U32)


def _running_max(a):
    return np.maximum.accumulate(np.asarray(a, dtype=U32)) if len(a) else np.zeros(0, U32)


def sort_batch(c, sl, keys, pos, hints=True, small=True, medium=True, tail=True, stats=None):
    """(sorted records, lcp hints): the elements of a batch -- first keys and records, in text order -- sorted completely by the
    model's own steps: first sort, heads0, gather_active, resolve_small, medium_groups + resolve_medium, then rounds of
    round_keys / tile_bounds / local_sort (+ range_groups for the long ranges) / round_heads / round_apply / round_compact, the
    tail finished by resolve_small(limit 1024).  The two library sorts of the product (radix sort of the first keys, segmented
    sort of the long ranges) are numpy's stable sort.  stats (optional dict): how often each step ran."""
    B = len(keys)
    stats = {} if stats is None else stats
    def ran(what, by=1):
        stats[what] = stats.get(what, 0) + by
    lcp = np.full(B, 0xFFFFFFFF, U32) if hints else None
    order = np.argsort(np.asarray(keys, dtype=U64), kind="stable")
    key_b, out = np.asarray(keys, dtype=U64)[order], np.asarray(pos, dtype=U64)[order].copy()
    head, active, lcp = heads0(key_b, c.bits, c.chars, np.zeros(B, U8), np.zeros(B, U8), lcp)
    idx = _select(active, B)
    m = len(idx)
    if not m:
        return out, lcp
    err = np.zeros(16, U32)
    slot, p, hv = gather_active(idx, out, head, np.zeros(m, U32), np.zeros(m, U64), np.zeros(m, U32))
    ghead = _running_max(hv)
    offset = c.chars

    def compact(keep, slot, p, ghead):
        s2, p2, h2 = round_compact(keep, slot, p, ghead, np.zeros(len(keep), U32), np.zeros(len(keep), U64), np.zeros(len(keep), U32))
        return s2, p2, _running_max(h2)
    if small:
        out, flags, err, lcp = resolve_small(c, p, ghead, slot, offset, out, np.zeros(m, U8), err, lcp)
        ran("small", int((flags == 0).sum()))
        keep = _select(flags, m)
        if len(keep) and len(keep) < m:
            slot, p, ghead = compact(keep, slot, p, ghead)
        m = len(keep)
        if m and medium:
            regions, counts = medium_groups(ghead[:m])
            if sum(counts):
                out, flags, err, lcp = resolve_medium(c, sl, p, slot, regions, offset, out, np.ones(m, U8), err, lcp)
                ran("medium", int((flags == 0).sum()))
                keep = _select(flags, m)
                if len(keep) and len(keep) < m:
                    slot, p, ghead = compact(keep, slot, p, ghead)
                m = len(keep)
    tail_done = False
    target, limit = 1024, SORT_CAP - 1024
    while m:
        ran("rounds")
        assert stats["rounds"] < 1000
        ka, _ = round_keys(c, p[:m], offset, np.zeros(m, U64), err)
        n_tiles = (m + target - 1) // target
        bound = tile_bounds(ghead[:m], target, limit, n_tiles, np.zeros(n_tiles + 1, U32))
        kb, pc_, big, _ = local_sort(ka, p[:m], ghead[:m], bound, ka.copy(), p[:m].copy(), 1 << 30)
        if big:
            for b, e in range_groups(ghead[:m], [x for x, _ in big], [y for _, y in big]):
                o = np.argsort(ka[b:e], kind="stable")
                kb[b:e], pc_[b:e] = ka[b:e][o], p[b:e][o]
            ran("long ranges", len(big))
        hv, err, lcp = round_heads(c, kb, ghead[:m], np.zeros(m, U32), err, lcp, slot[:m] if hints else None, offset)
        hv = _running_max(hv)
        out, flags = round_apply(pc_, hv, slot[:m], out, np.zeros(m, U8))
        keep = _select(flags, m)
        if len(keep):
            slot, p, ghead = compact(keep, slot[:m], pc_, hv)
        m = len(keep)
        offset = (1 << 40) if c.giant is not None and offset >= c.g_depth else offset + c.chars
        if m and m <= 32768 and not tail_done and offset < (1 << 40) and tail:
            tail_done = True
            out, flags, err, lcp = resolve_small(c, p, ghead, slot, offset, out, np.zeros(m, U8), err, lcp, 1024)
            ran("tail", int((flags == 0).sum()))
            keep = _select(flags, m)
            if len(keep) and len(keep) < m:
                slot, p, ghead = compact(keep, slot, p, ghead)
            m = len(keep)
    assert not err[:3].any(), err[:3]
    return out, lcp
