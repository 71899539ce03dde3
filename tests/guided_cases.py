"""The named cases of tests/test_gpu_guided_kernels.py (the single launch wrappers of csrc/guided_kernels.hpp against
tests/guidedmodel.py), the wrappers that have no probe yet, and a mirror of the probe library's precondition checks
(tests/kprobe/kprobe.cpp, the need(...) lines of the kp_gk_* functions): tests/test_guided_model_host.py runs every case
through the mirror on the CPU, so that no designed case can be rejected -- and so silently not run -- on the GPU.

Cases are built at the boundaries the kernels' code names; each generator's docstring says which."""
import numpy as np

import guidedmodel as GM

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
NO_BOUND = GM.NO_BOUND
TILE = GM.TILE
MAX_TEXT = 5 * 4096 + 70

# Wrappers of guided_kernels.hpp without a probe and a model function: name -> reason.  The same names stand in the header
# of tests/test_gpu_guided_kernels.py; tests/test_guided_model_host.py checks both lists against the declarations.
NOT_COVERED = {}


# ---- phrase ends ---------------------------------------------------------------------------------------------------------
def cut_cases():
    """name -> (n, cuts).  Sizes 1, 4095, 4096, 4097, 3 * 4096 + 5; no cut at all; cuts at 0, 63, 64, 511, 512, 4095, 4096 and
    n - 1; an empty block followed by one whose first cut is at offset 0; blocks with 1, 8, 9, 64, 65 and 513 cuts (list_lower:
    the `hi - lo <= 8` exit, two and three levels of its 8-ary step)."""
    out = {}
    for n in (1, 4095, 4096, 4097, 3 * 4096 + 5):
        out["none_%d" % n] = (n, [])
        out["edges_%d" % n] = (n, sorted({p for p in (0, 63, 64, 511, 512, 4095, 4096, n - 1) if p < n}))
    out["gap_then_zero"] = (3 * 4096 + 5, [100, 4000, 2 * 4096, 2 * 4096 + 9])
    rng = np.random.default_rng(11)
    cuts = []
    for b, k in enumerate((1, 8, 9, 64, 65)):
        cuts += (b * TILE + np.sort(rng.choice(TILE, k, replace=False))).tolist()
    cuts += [5 * TILE + 3, 5 * TILE + 69]
    out["counts_1_8_9_64_65"] = (MAX_TEXT, cuts)
    dense = (np.sort(rng.choice(TILE, 513, replace=False))).tolist()
    out["counts_513"] = (3 * 4096 + 5, dense + [2 * TILE, 2 * TILE + 1, 3 * TILE + 4])
    return out


CUT_BLOCK_COUNTS = {"counts_1_8_9_64_65": [1, 8, 9, 64, 65, 2], "counts_513": [513, 0, 2, 1]}


# ---- first keys --------------------------------------------------------------------------------------------------------------
def pack_key(symbols, bits):
    k = 0
    for s in symbols:
        k = (k << bits) | s
    return k


def heads0_cases():
    """name -> (keys sorted ascending, bits, chars).  B = 1, 2, 256, 257; all equal; all distinct; neighbours that differ in
    every symbol position from the first to the last, with bits * chars = 63 (3 x 21: keys with bit 62 set) and = 60 (3 x 20)."""
    out = {}
    for bits, chars in ((3, 21), (3, 20)):
        tag = "_%d" % (bits * chars)
        top = pack_key([7] * chars, bits)
        for B in (1, 2, 256, 257):
            out["equal_B%d%s" % (B, tag)] = (np.full(B, top - 5, U64), bits, chars)
            out["distinct_B%d%s" % (B, tag)] = (np.arange(B, dtype=U64) * U64(3) + U64(top - 3 * 257), bits, chars)
        # a chain: every key twice (groups of two); the next one differs from it first at symbol chars - 1 - i, i = 0 .. chars - 1
        keys = []
        sym = [1] * chars
        for i in range(chars):
            keys += [pack_key(sym, bits)] * 2
            sym = list(sym)
            sym[chars - 1 - i] = 7 if i == chars - 1 else 2 + (i % 5)
            for j in range(chars - i, chars):
                sym[j] = 0
        keys += [pack_key(sym, bits)]
        assert keys == sorted(keys)
        out["chain" + tag] = (np.array(keys, dtype=U64), bits, chars)
    return out


# ---- groups ----------------------------------------------------------------------------------------------------------------
def gheads(sizes):
    out = []
    for s in sizes:
        out += [len(out)] * s
    return np.array(out, dtype=U32)


MEDIUM_SIZES = (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)


def medium_cases():
    """name -> (sizes, cap).  Every size at a class boundary (9, 16 | 17, 32 | 33, 64 | 65, 128 | 129: not listed); more than
    1024 elements (the kernel's workgroups take 1024 each: groups across that line, several allocations per class); a region
    filled to its last pair; a list that ends with a group of 129 and one that ends with a group of 9."""
    out = {"each_size": (list(MEDIUM_SIZES), 5)}
    rng = np.random.default_rng(5)
    many = [int(MEDIUM_SIZES[i]) for i in rng.integers(0, len(MEDIUM_SIZES), 120)]
    counts = [sum(1 for s in many if GM.medium_class(s) == cl) for cl in range(4)]
    out["many_exact_cap"] = (many, max(counts))
    out["ends_with_129"] = ([9, 130, 16, 129], 2)
    out["ends_with_9"] = ([129, 128, 9], 1)
    out["one_element"] = ([1], 1)
    return out


def bounds_cases():
    """name -> (sizes, target, limit, n_tiles).  A head exactly at t * target; `limit` reached (NO_BOUND); m not a multiple of
    target; a tile that begins at or beyond m; the stretch that reaches m without a head."""
    return {
        "exact_heads": ([8, 8, 8, 8], 8, 8, 4),
        "limit_reached": ([3, 40, 5, 2], 8, 8, 7),
        "ragged_m": ([5, 6, 7, 3], 8, 16, 3),
        "beyond_m": ([4, 4], 8, 8, 3),
        "tail_without_head": ([2, 30], 8, 64, 4),
        "limit_one_short": ([1, 16, 3], 8, 8, 3),       # the head at 17 = 8 + 9: just outside [8, 16)
        "limit_just_reaches": ([1, 15, 4], 8, 9, 3),    # the head at 16 = 8 + 8: the last position of [8, 17)
    }


class SortCase:
    """the input of local_sort: groups, keys, records, forged bounds (a bound is a group's head, m or NO_BOUND)"""

    def __init__(self, name, tiles, seed, key_range, trailing_none=0, empty_tile=False):
        rng = np.random.default_rng(seed)
        sizes, bound = [], []
        at = 0
        for groups in tiles:
            bound.append(at)
            n_el = sum(groups)
            sizes += groups
            at += n_el
            bound += [NO_BOUND] * ((n_el - 1) // GM.SORT_CAP)        # a long tile is followed by tiles that begin inside it
            if empty_tile:
                bound.append(at)                                      # two tiles that found the same head: the first is empty
        bound += [NO_BOUND] * trailing_none                           # tiles that begin inside the last group
        bound.append(at)
        self.name = name
        self.sizes = sizes
        self.ghead = gheads(sizes)
        self.m = at
        self.bound = np.array(bound, dtype=U32)
        self.kin = rng.integers(0, key_range, self.m).astype(U64) | (U64(1) << U64(63)) * (rng.integers(0, 2, self.m).astype(U64))
        self.pin = (np.arange(self.m, dtype=U64) * U64(0x10001)) ^ U64(0x5A5A00000000)     # distinct records
        self.n_big = sum(1 for g in tiles if sum(g) > GM.SORT_CAP)


def sort_cases():
    """Tiles of 1, 2047, 2048 and 2049 elements (the last is listed as big); groups of 64 and 65 (SHORT: the network); equal keys
    inside a group on both paths; tiles behind NO_BOUND bounds; an empty tile; two big tiles (for a big_cap one short)."""
    count_2047 = [64] * 31 + [63]
    net_2048 = [65] + [64] * 30 + [63]
    return [
        SortCase("sizes", [[1], count_2047, net_2048, [2049], [5, 3]], 3, 40),
        SortCase("two_big", [[2, 2], [1500, 1500], [64, 64], [4097], [65]], 4, 7, trailing_none=2),
        SortCase("equal_keys", [[64] * 4, [65] * 4, [2048]], 5, 1),
        SortCase("empty_tiles", [[3], [70, 2], [1]], 6, 1000, empty_tile=True),
    ]


def range_cases():
    """name -> (sizes, [(begin, end)]).  A range that is one group; a range of many groups (more than 1024 elements: a workgroup's
    stretch, and more than 64 * 1024: every stretch of the 64 is used); a range that ends inside a group; an empty range."""
    return {
        "one_group": ([5, 3000, 2], [(5, 3005)]),
        "many_groups": ([2, 3] * 500 + [1100, 2], [(0, 2500), (2500, 3602)]),
        "cut_group": ([10, 10, 10], [(0, 15), (20, 30)]),
        "empty_range": ([4, 4], [(4, 4), (0, 8)]),
        "long_range": ([2] * 35000, [(0, 70000)]),
    }


# ---- the probe's preconditions, mirrored ------------------------------------------------------------------------------------
def gheads_ok(ghead):
    return all(int(g) == c or (c > 0 and int(g) == int(ghead[c - 1]) and int(g) < c) for c, g in enumerate(ghead))


def reject_block_cut_offsets(mask, brank, n_blocks, alloc):
    for b in range(n_blocks):
        c = sum(GM._popcount(x) for x in mask[64 * b:64 * (b + 1)])
        if int(brank[b]) + c > alloc:
            return "brank + the block's cuts beyond coff"
    return None


def reject_medium_groups(ghead, cap, alloc):
    if not gheads_ok(ghead):
        return "ghead: every element names the first of its group"
    if alloc < 4 * cap:
        return "count4 holds 4 words, list 4 regions of cap pairs"
    if any(c > cap for c in GM.medium_groups(ghead)[1]):
        return "a class has more groups than a region holds"
    return None


def reject_local_sort(ghead, bound, big_cap, big_alloc):
    m = len(ghead)
    if big_cap > big_alloc or len(bound) < 2:
        return "big_cap within the lists, a tile at least"
    if not gheads_ok(ghead):
        return "ghead: every element names the first of its group"
    if int(bound[-1]) == NO_BOUND:
        return "the last bound ends every search"
    for b in bound:
        b = int(b)
        if not (b == NO_BOUND or (b <= m and (b == m or int(ghead[b]) == b))):
            return "a bound is a group's head or m"
    return None


def reject_range_groups(ghead, begins, ends, seg_alloc):
    if not len(begins):
        return "a range at least"
    if not gheads_ok(ghead):
        return "ghead: every element names the first of its group"
    if any(not (b <= e <= len(ghead)) for b, e in zip(begins, ends)):
        return "a range within the list"
    if len(GM.range_groups(ghead, begins, ends)) > seg_alloc:
        return "more groups than the segment lists hold"
    return None


def reject_index(idx, limit, what):
    return what if any(int(i) >= limit for i in idx) else None


# ---- texts and contexts of the kernels that read gk::Ctx ------------------------------------------------------------------------
ALPHABET = b"$ACGNT"                      # with the Dollar (0x02): seven symbols, three bits, 21 characters a key (bit 62 in use)


def full_code():
    """(code, bits, chars) of the seven symbols: Dollar 1, '$' 2, A 3, C 4, G 5, N 6, T 7 -- N lies between two bases"""
    return GM.code_table(np.frombuffer(ALPHABET, U8))


def _bases(rng, n, letters=b"ACGT"):
    return np.frombuffer(letters, U8)[rng.integers(0, len(letters), n)].copy()


def text_cases():
    """name -> text.  n = 4096 k - 1, 4096 k, 4096 k + 1 (k = 1, 3); the last full tile with exactly 63 and exactly 64 plain
    characters behind it (the dense tiles' condition base + TILE + 64 <= n); an exception in the last position of a tile, in the
    first of the next, 63 and 64 positions into the next; a tile of one symbol; runs of T that end inside a tile, at a tile's last
    position, that span one, two and three whole tiles and that reach the end of the text, followed by symbols below and above T;
    an alphabet without G (no dense tiles at all)."""
    rng = np.random.default_rng(77)
    out = {}
    for k in (1, 3):
        for d in (-1, 0, 1):
            out["n=%dx4096%+d" % (k, d)] = _bases(rng, 4096 * k + d)
    out["plain63"] = _bases(rng, 2 * 4096 + 63)
    out["plain64"] = _bases(rng, 2 * 4096 + 64)
    for at, byte in ((4095, b"N"), (4096, b"$"), (4096 + 63, b"N"), (4096 + 64, b"$")):
        t = _bases(rng, 3 * 4096 + 70)
        t[at] = byte[0]
        out["exception@%d" % at] = t
    t = _bases(rng, 5 * 4096 + 70)
    t[4096:2 * 4096] = ord("T"); t[4095] = ord("G"); t[2 * 4096] = ord("A")                 # tile 1 is T only: a run of one whole tile
    t[3 * 4096 - 40:3 * 4096] = ord("N")                                                    # N^40 up to a tile's last position
    t[3 * 4096 + 100:3 * 4096 + 130] = ord("N"); t[3 * 4096 + 130] = ord("T")               # N^30 followed by a symbol above N
    t[3 * 4096 + 500:3 * 4096 + 800] = ord("N"); t[3 * 4096 + 800] = ord("A")               # N^300 (r >= 256) followed by one below
    out["runs"] = t
    t = _bases(rng, 5 * 4096 + 70)
    t[2000:2000 + 2 * 4096 + 2096] = ord("T"); t[1999] = ord("A")                           # spans tiles 1 and 2 whole, ends at 12287
    t[4 * 4096 + 10:] = ord("T"); t[4 * 4096 + 9] = ord("C")                                 # reaches the end of the text
    out["long_runs"] = t
    t = _bases(rng, 4 * 4096 + 33)
    t[50:50 + 3 * 4096 + 4000] = ord("N"); t[49] = ord("T"); t[50 + 3 * 4096 + 4000] = ord("T")   # N over three whole tiles
    out["n_run_3_tiles"] = t
    t = _bases(rng, 4096 + 200, b"ACT")
    t[300:320] = ord("N")
    out["no_G"] = t
    return out


def forged_cuts(n, w, seed, mean=60):
    """phrase ends of a made-up parse: gaps of w .. 2 mean characters (a tile holds tens to hundreds of phrases), and a stretch
    without any (a giant phrase) where the text is long enough"""
    rng = np.random.default_rng(seed)
    cuts, at = [], int(rng.integers(w, 2 * mean))
    while at < n:
        if not (5000 <= at < 5700):
            cuts.append(at)
        at += int(rng.integers(w, 2 * mean))
    return cuts


def make_ctx(text, w=6, seed=1, rec="len", rep=None, skip=0, expand=0, code=None, **kw):
    """a model context over forged phrase ends.  rec: "len" (records carry |alpha|) or "rank" (the rank that follows, above
    pos_bits = 20 bits); rep: None, "all" or "alternate" """
    n = len(text)
    cuts = forged_cuts(n, w, seed)
    m = len(cuts) + 1
    rng = np.random.default_rng(seed + 1000)
    code, bits, chars = full_code() if code is None else code
    flags = None if rep is None else ([1] * m if rep == "all" else [k & 1 for k in range(m)])
    return GM.Ctx(text, w, cuts, code, bits, chars, skip=skip, pos_bits=20 if rec == "rank" else 40, rec_rank=1 if rec == "rank" else 0,
                  isa_p=rng.permutation(m).astype(U32), pid=(rng.integers(0, max(1, m // 2), m)).astype(U32), rep=flags, expand=expand, **kw)


def bin_ranges(c, pc):
    """[(lo, hi)] for prefix_chars = pc: empty, full, one that starts and ends on bins that are not all bases (N: between G and
    T; Dollar and '$': below A), one from a '$' bin to an N bin, one that starts and ends on all-base bins, the single bin T^pc"""
    code = c.code
    def b(s):
        v = 0
        for ch in s:
            v = (v << c.bits) | int(code[ch])
        return v
    A, C_, G, N, T, S = (bytes([x]) for x in b"ACGNT$")
    full = 1 << (c.bits * pc)
    return [(7, 7), (0, full), (b((G + N + A * pc)[:pc]), b((T + N + A * pc)[:pc])), (b((S + A * pc)[:pc]), b((N + A * pc)[:pc])),
            (b((C_ * pc)[:pc]), b((G + T * pc)[:pc]) + 1), (b(T * pc), b(T * pc) + 1)]


def real_giant(c):
    """the dictionary of the context's phrases longer than g_depth, but for every third of them (long phrases outside the
    dictionary: members that clear a group's `pure`)"""
    longs = [k for k in range(c.m) if c.phrase_len(k) > c.g_depth]
    left_out = set(longs[2::3])
    return GM.derive_giant(c, keep=lambda k: k not in left_out)


# ---- loci: copies of one segment with planted substitutions, for the kernels that compare phrase suffixes --------------------------
SPACER, SEGMENT = 40, 400


class Locus:
    """n copies of a random segment of 400 bases, each behind a spacer of its own; copy i carries substitutions at the segment
    positions muts[i] and ONE phrase end inside the segment, at position ends[i] (a forged parse: the ends need not agree).
    Every copy has one more phrase end at segment position 12, so that the phrase behind it is the same distinct phrase in the
    copies that carry no substitution inside it (pid says so, by the phrases' bytes).
    members(s): the records of the suffixes at segment position s >= 12 of every copy -- a group that shares the characters up to
    the first substitution at or behind s; |alpha| = ends[i] - s + 1."""

    def __init__(self, muts, ends, seed=1, w=6, rec="len", expand=0, ranks=None, skip=0, g_depth=0, n_at=None):
        rng = np.random.default_rng(seed)
        seg = _bases(rng, SEGMENT)
        nxt = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}
        parts, cuts, self.starts = [], [], []
        for i, (mu, end) in enumerate(zip(muts, ends)):
            sp = _bases(rng, SPACER)
            sp[-1] = b"ACGT"[i % 4]; sp[-2] = b"ACGT"[(i // 4) % 4]; sp[-3] = b"ACGT"[(i // 16) % 4]; sp[-4] = b"ACGT"[(i // 64) % 4]
            s = seg.copy()
            for x in mu:
                s[x] = nxt[int(seg[x])]
            for x in (n_at or {}).get(i, ()):                             # an exception (N) in this copy alone
                s[x] = ord("N")
            at = sum(len(p) for p in parts)
            cuts += [at + 10, at + SPACER + 12, at + SPACER + end]       # (one end at segment position 12: the phrases behind it repeat)
            self.starts.append(at + SPACER)
            parts += [sp, s]
        text = np.concatenate(parts + [_bases(rng, 30)])
        m = len(cuts) + 1
        isa = np.random.default_rng(seed + 7).permutation(m).astype(U32) if ranks is None else np.asarray(ranks, dtype=U32)
        code, bits, chars = full_code()
        self.c = GM.Ctx(text, w, cuts, code, bits, chars, pos_bits=20 if rec == "rank" else 40, rec_rank=1 if rec == "rank" else 0,
                        isa_p=isa, pid=np.zeros(m, U32), expand=expand, skip=skip, g_depth=g_depth)
        if g_depth:                                                       # the real dictionary of the phrases longer than g_depth
            self.c.giant = GM.derive_giant(self.c)
        spelled = {}
        for k in range(m):                                                # ids of the distinct phrases, by their bytes
            a = self.c.phrase_start(k)
            self.c.pid[k] = spelled.setdefault(bytes(self.c.vbyte(a + t) for t in range(self.c.phrase_len(k))), len(spelled))
        self.ends = list(ends)

    def phrases(self):
        """the records of the phrase that begins behind segment position 12, one per copy (lists of phrases: skip = 1)"""
        return np.array([self.c.make_rec(self.c.phrase_start(3 * i + 2)) for i in range(len(self.starts))], dtype=U64)

    def members(self, s):
        return np.array([self.c.make_rec(st + s + 1) for st in self.starts], dtype=U64)


def pair_cases(offset=21, s=30, L=150):
    """name -> (muts, ends): two copies that part at offset + 0, 7, 8, 31 (the four words the pair path loads), + 32 (the walk
    behind them), + 63, 64, 65, exactly at the last character of alpha, not at all (the same alpha: the ranks decide), and with
    alphas of two lengths that agree up to the shorter one (forged ends: err[1])"""
    end = s + L - 1
    out = {"differ_at_+%d" % d: ([[], [s + offset + d]], [end, end]) for d in (0, 7, 8, 31, 32, 63, 64, 65)}
    out["differ_at_L-1"] = ([[], [end]], [end, end])
    out["differ_behind_L"] = ([[], [end + 1]], [end, end])
    out["same_alpha"] = ([[], []], [end, end])
    out["two_lengths"] = ([[], []], [end, end - 40])
    out["short_alpha_L=offset+5"] = ([[], [s + offset + 2]], [s + offset + 4, s + offset + 4])
    return out


def reject_compared(c, recs, offset):
    qs = [c.rec_pos(r) for r in recs]
    if reject_elements(c, qs):
        return reject_elements(c, qs)
    if any(offset > c.rec_len(r) or c.rec_pos(r) + c.rec_len(r) > c.n + 40 for r in recs):
        return "alpha inside V, the shared prefix inside alpha"
    return None


def medium_layouts(staged, s=30, offset=21, L=300):
    """name -> (per-copy substitutions for four kinds of copies, how many of each): the copies of one locus.  `staged` = the
    characters the kernel stages behind `offset` (64; 32 for the class of 128): the third shared difference lies just before,
    at and just behind them."""
    a, b = s + offset + 5, s + offset + 11
    out = {"all_equal": [[]],
           "one_private": [[], [a]],
           "two_share_one": [[], [a], [a]],
           "short_alpha": [[], [a]]}
    for d in (-1, 0, 1):
        out["two_share_two_third_at_staged%+d" % d] = [[], [a, b], [a, b, s + offset + staged + d]]
    return out


def three_base_text():
    """three tiles and 70 characters of A, C and T alone: every tile but the last could be read as 2-bit words -- with the text's
    own code table G has no code, and that alone keeps every tile on the staged path"""
    return _bases(np.random.default_rng(78), 3 * 4096 + 70, b"ACT")


def reject_elements(c, qs):
    return None if all(q <= c.n and (q >= 1 or c.skip) for q in qs) else "an element's V index is 1 .. n (0: the first phrase)"


def reject_ctx(c, pc=None):
    """the context's own preconditions (the probe library's DevCtx and need_text_order)"""
    if not (c.n >= 1 and 1 <= c.w <= 32):
        return "n = text length >= 1, 1 <= w <= 32"
    if not (c.bits >= 1 and c.chars >= 1 and c.bits * c.chars <= 63):
        return "1 <= bits * chars <= 63"
    if int(c.code[0]) != 0:
        return "a code table (code[0] = 0) and nxt"
    if not (1 <= c.pos_bits <= 63 and (c.rec_rank or c.pos_bits == 40)):
        return "pos_bits 1 .. 63, 40 when the records carry lengths"
    if any(int(x) > c.n + c.w - 1 for x in c.t.nxt):
        return "nxt at most n + w - 1"
    if c.cuts and c.cuts[-1] >= c.n:
        return "phrase ends below n"
    if c.isa_p is None and not c.skip and not c.expand:
        return "isa_p unless the elements are phrases or representatives"
    if pc is not None and not (not c.skip and 1 <= pc <= c.chars and c.bits * pc <= 20):
        return "text suffixes; 1 <= prefix_chars <= chars, bins of at most 20 bits"
    return None
