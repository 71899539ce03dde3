"""ctypes / numpy side of tests/kprobe/libkprobe.so (single launch wrappers of the suffix sorter and of the prefix-free parse
behind C functions), the plain references the sorter's kernel tests compare with, the generator of legal active lists, and
(at the end) the texts, the packer and the thin wrappers of the parse's probes, whose references are tests/pfpmodel.py, and
of the bucket-wise producer's (gk_*, with the context structure KpCtx), whose references are tests/guidedmodel.py.

Everything in the references is integer arithmetic on numpy arrays or Python ints: there is no tolerance anywhere.
The references import nothing from the product; tests/test_sorter_reference_host.py checks them (and the generator)
on the CPU, so that a broken reference cannot make a GPU test pass vacuously.
"""
import contextlib
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "kprobe", "libkprobe.so")
NO_SEP = 0xFFFFFFFF
NO_BOUND = 0xFFFFFFFF
U32, U64, U8 = np.uint32, np.uint64, np.uint8
SENT32 = 0xA5A5A5A5            # fill patterns of in/out arrays: what a wrapper must not touch comes back as this
SENT64 = 0xA5A5A5A5A5A5A5A5
SENT8 = 0xA5

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.kp_last_error.restype = ctypes.c_char_p
        _lib.kp_round_fused_cap.restype = ctypes.c_uint32
        _lib.kp_round_tile_cap.restype = ctypes.c_uint32
    return _lib


class ProbeError(RuntimeError):
    pass


def _arg(a):
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(ctypes.c_void_p)
    if a is None:
        return ctypes.c_void_p(0)
    return a


def call(name, *args):
    """kp_<name>(*args): numpy arrays go as pointers, Python ints as 32-bit values (ctypes' default), None as NULL."""
    fn = getattr(lib(), "kp_" + name)
    rc = fn(*[_arg(a) for a in args])
    if rc != 0:
        raise ProbeError("kp_%s: %s" % (name, lib().kp_last_error().decode()))


@contextlib.contextmanager
def environment(**values):
    """environment variables for the calls inside the block (live switches are read at every call), then as they were"""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def u32(x):
    return np.ascontiguousarray(x, dtype=U32)


def u64(x):
    return np.ascontiguousarray(x, dtype=U64)


def u8(x):
    return np.ascontiguousarray(x, dtype=U8)


def c_u32(v):
    return ctypes.c_uint32(int(v) & 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------
# thin wrappers (shapes and sentinels in one place)
# ---------------------------------------------------------------------------------------------------------------------
def pack_keys(text, code, bits, chars, sep_code=NO_SEP, run_alloc=0, run_cap=0):
    text = u8(text); n = len(text)
    keys = np.empty(n, U64); vals = np.empty(n, U32)
    if run_alloc:
        ends = np.full(run_alloc, SENT32, U32); cnt = np.zeros(1, U32)
        call("pack_keys", text, n, u8(code), bits, chars, c_u32(sep_code), keys, vals, ends, run_alloc, cnt, run_cap)
        return keys, vals, ends, int(cnt[0])
    call("pack_keys", text, n, u8(code), bits, chars, c_u32(sep_code), keys, vals, None, 0, None, 0)
    return keys, vals


def pack_keys_u32(parse, bits, chars):
    parse = u32(parse); m = len(parse)
    keys = np.empty(m, U64); vals = np.empty(m, U32)
    call("pack_keys_u32", parse, m, bits, chars, keys, vals)
    return keys, vals


def scan(which, a, out_dtype):
    a = np.ascontiguousarray(a); out = np.empty(len(a), out_dtype)
    call("scan", which, a, out, len(a))
    return out


def sort_ranges(kin, vin, begin, end, end_bit, ordered=False):
    """(kout, vout), both pre-filled with the sentinel pattern"""
    kin = np.ascontiguousarray(kin); vin = np.ascontiguousarray(vin)
    kout = np.full(len(kin), SENT64 if kin.itemsize == 8 else SENT32, kin.dtype)
    vout = np.full(len(vin), SENT64 if vin.itemsize == 8 else SENT32, vin.dtype)
    call("sort_ranges", kin.itemsize, vin.itemsize, kin, vin, kout, vout, len(kin), len(begin), u32(begin), u32(end), end_bit,
         1 if ordered else 0)
    return kout, vout


def sorter_text(text, code, bits, chars, sigma, sep_code=NO_SEP, use_runs=False):
    text = u8(text); n = len(text)
    sa = np.empty(n, U32); rank = np.empty(n, U32); out = np.zeros(2, U64)
    call("sorter_text", text, n, u8(code), bits, chars, sigma, c_u32(sep_code), 1 if use_runs else 0, sa, rank, out)
    return sa, rank, int(out[0]), int(out[1])


def sorter_ints(parse, bits, chars):
    parse = u32(parse); m = len(parse)
    sa = np.empty(m, U32); rank = np.empty(m, U32); out = np.zeros(2, U64)
    call("sorter_ints", parse, m, bits, chars, sa, rank, out)
    return sa, rank, int(out[0])


# ---------------------------------------------------------------------------------------------------------------------
# references: first keys
# ---------------------------------------------------------------------------------------------------------------------
def bit_width(v):
    return int(v).bit_length()


def ref_pack_keys(sym, bits, chars, sep_code=NO_SEP):
    """sym: symbol codes of the text.  key[i] = the first `chars` symbols of suffix i, big-endian, 0 past the end.  With a
    separator: (symbols up to and including the first separator of the window, zero behind it) << 1 | 1, else key << 1."""
    n = len(sym)
    s = [int(x) for x in sym] + [0] * (chars + 1)
    keys = np.empty(n, U64)
    for i in range(n):
        k = 0
        hit = False
        for c in range(chars):
            x = 0 if hit else s[i + c]
            k = (k << bits) | x
            if not hit and sep_code != NO_SEP and s[i + c] == sep_code:
                hit = True
        if sep_code != NO_SEP:
            k = (k << 1) | (1 if hit else 0)
        keys[i] = k
    return keys


def ref_pack_keys_u32(parse, bits, chars):
    m = len(parse)
    s = [int(x) for x in parse] + [0] * chars
    keys = np.empty(m, U64)
    for i in range(m):
        k = 0
        for c in range(chars):
            k = (k << bits) | s[i + c]
        keys[i] = k
    return keys


def ref_run_ends(sym, chars):
    """last positions of the maximal runs of `chars` or more equal non-zero symbols"""
    out = []
    n = len(sym)
    i = 0
    while i < n:
        j = i
        while j + 1 < n and sym[j + 1] == sym[i]:
            j += 1
        if sym[i] != 0 and j - i + 1 >= chars:
            out.append(j)
        i = j + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# references: heads and ranks (the one-line definitions of kernels.hpp)
# ---------------------------------------------------------------------------------------------------------------------
def ref_mark_heads(keys, lsb_unique):
    keys = u64(keys); n = len(keys)
    j = np.arange(n, dtype=U32)
    is_head = np.ones(n, bool)
    is_head[1:] = keys[1:] != keys[:-1]
    if lsb_unique:
        is_head |= (keys & U64(1)) == 1
    return np.where(is_head, j, U32(0)).astype(U32)


def ref_running_max(a):
    return np.maximum.accumulate(np.asarray(a))


def ref_flag_unsorted(head):
    head = u32(head); n = len(head)
    own = head == np.arange(n, dtype=U32)
    nxt = np.ones(n, bool)
    nxt[:-1] = own[1:]
    return (~(own & nxt)).astype(U8)


def ref_mark_subheads(keys, pos):
    keys = u64(keys); m = len(keys)
    is_head = np.ones(m, bool)
    is_head[1:] = keys[1:] != keys[:-1]
    return np.where(is_head, u32(pos), U32(0)).astype(U32)


def ref_round_flags(newhead, pos):
    """flags[c] = 0 iff element c is a bucket of its own: newhead[c] == pos[c] and the next element (if any) is a head"""
    newhead = u32(newhead); pos = u32(pos); m = len(pos)
    own = newhead == pos
    nxt = np.ones(m, bool)
    nxt[:-1] = own[1:]
    return (~(own & nxt)).astype(U8)


def ref_round_keys(sac, headc, rank, n, h, shift):
    """keys[c] = head[c] << shift | (rank[sa[c] + h] + 1, or 0 past the end); Python ints: no width to overflow"""
    out = np.empty(len(sac), U64)
    for c in range(len(sac)):
        i = int(sac[c]) + int(h)
        second = int(rank[i]) + 1 if i < n else 0
        out[c] = ((int(headc[c]) << shift) | second) & 0xFFFFFFFFFFFFFFFF
    return out


def ref_equal_range(sorted_keys, probe):
    s = [int(x) for x in sorted_keys]
    out = []
    for p in probe:
        p = int(p)
        out += [sum(1 for x in s if x < p), sum(1 for x in s if x <= p)]
    return u32(out)


# ---------------------------------------------------------------------------------------------------------------------
# the generator of legal active lists
# ---------------------------------------------------------------------------------------------------------------------
class ActiveList:
    """The input of a doubling round: m tied suffixes grouped by bucket.  pos[c] = suffix-array position (ascending),
    sac[c] = the suffix there, headc[c] = position of its bucket's first element (head <= pos, a bucket's positions are
    consecutive), rank = the rank column (rank[sa[j]] = head of j's bucket; a position outside every bucket is a
    bucket of its own), sa = the suffix array so far, n its length."""

    def __init__(self, sizes, gaps, tail=0, seed=1):
        assert len(sizes) == len(gaps) and all(s >= 2 for s in sizes) and all(g >= 0 for g in gaps)
        rng = np.random.default_rng(seed)
        pos, headc = [], []
        head_of = []
        cur = 0
        for s, g in zip(sizes, gaps):
            head_of += list(range(cur, cur + g))
            cur += g
            pos += list(range(cur, cur + s)); headc += [cur] * s
            head_of += [cur] * s
            cur += s
        head_of += list(range(cur, cur + tail))
        self.n = cur + tail
        self.m = len(pos)
        self.sizes = list(sizes)
        self.pos = u32(pos); self.headc = u32(headc)
        self.sa = u32(rng.permutation(self.n))
        self.head = u32(head_of)
        self.sac = self.sa[self.pos]
        self.rank = np.empty(self.n, U32)
        self.rank[self.sa] = self.head
        self.shift = bit_width(self.n)

    def check(self):
        n, m = self.n, self.m
        assert m == sum(self.sizes) and len(self.pos) == m and len(self.sac) == m and len(self.headc) == m
        assert np.all(self.pos[1:] > self.pos[:-1]) and (m == 0 or int(self.pos[-1]) < n)
        assert np.all(self.headc <= self.pos)
        assert sorted(self.sa.tolist()) == list(range(n))
        assert np.array_equal(self.sac, self.sa[self.pos])
        assert np.array_equal(self.rank[self.sac], self.headc)
        c = 0
        for s in self.sizes:                               # buckets contiguous, in order, head = first position
            assert np.all(self.headc[c:c + s] == self.pos[c]) and np.array_equal(self.pos[c:c + s], self.pos[c] + np.arange(s, dtype=U32))
            if c:
                assert self.headc[c] != self.headc[c - 1]
            c += s
        assert np.array_equal(ref_flag_unsorted(self.head)[self.pos], np.ones(m, U8))       # every member is tied
        assert int(ref_flag_unsorted(self.head).sum()) == m                                   # and nothing else is
        return True


def round_shapes(cap):
    """The bucket lists the issue names, for a tile capacity `cap` (target = cap / 2): name -> (sizes, gaps, tail)."""
    t = cap // 2
    few = [2, 3, 5, 2, 7, 2]
    return {
        "short_edge": ([2, 128, 129, 2, 128, 2] + few, [1, 0, 3, 0, 0, 2] + [1] * len(few), 5),
        "target_edge": ([t - 1, t, t + 1, 2, t, t - 1, 3], [0, 1, 0, 0, 2, 0, 0], 1),
        "cap_edge": ([cap - 1, 2, cap, 3, cap + 1, 2, 2], [0, 0, 1, 0, 0, 0, 4], 2),
        "four_tiles": ([3, 5 * t + 7, 2, 2], [0, 2, 0, 1], 3),           # four whole tiles inside: three bounds in a row are "none"
        "ends_at_m": ([5, t + 9, 4 * t], [1, 0, 0], 0),                    # the last bucket ends exactly at m (= n)
        "last_tile_one_bucket": ([2] * (t // 2) + [t - 3], [0] * (t // 2) + [0], 0),
        "many_long": ([cap + 1, 2, cap + 5, cap + 2, 3, 2 * cap + 1], [0, 0, 0, 1, 0, 0], 0),
    }


def ref_bounds(headc, target, limit, n_tiles):
    """bound[t] = first bucket start at or after t * target, NO_BOUND when none within `limit` elements; bound[0] = 0,
    bound[n_tiles] = m; a start at or beyond m reads m"""
    headc = u32(headc); m = len(headc)
    start = np.ones(m, bool)
    start[1:] = headc[1:] != headc[:-1]
    starts = np.flatnonzero(start)
    out = np.empty(n_tiles + 1, U32)
    for t in range(n_tiles + 1):
        if t == 0:
            out[t] = 0
        elif t == n_tiles:
            out[t] = m
        else:
            c0 = t * target
            stop = min(c0 + limit, m)
            k = np.searchsorted(starts, c0)
            c = int(starts[k]) if k < len(starts) else m
            if c >= stop:
                out[t] = m if stop >= m else NO_BOUND
            else:
                out[t] = c
    return out


def ref_ranges(bound, cap):
    """the ranges between consecutive bounds: [(tile, end tile, begin, end, long)] of the non-empty ones"""
    out = []
    n_tiles = len(bound) - 1
    for t in range(n_tiles):
        b = int(bound[t])
        if b == NO_BOUND:
            continue
        u = t + 1
        while int(bound[u]) == NO_BOUND:
            u += 1
        e = int(bound[u])
        if e > b:
            out.append((t, u, b, e, e - b > cap))
    return out


def ref_tile_big(bound, cap):
    n_tiles = len(bound) - 1
    marks = np.zeros(n_tiles + 1, U8)
    for t, u, b, e, long_ in ref_ranges(bound, cap):
        if long_:
            for x in range(t, u):
                marks[x] = 1 | (2 if x == t else 0) | (4 if x + 1 == u else 0)
    return marks


def ref_round(al, h):
    """One doubling round of the whole list: (sorted keys, new heads, flags, per element the (key -> set of suffixes))."""
    keys = ref_round_keys(al.sac, al.headc, al.rank, al.n, h, al.shift)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    # buckets are contiguous and their heads ascend, so the global order by key keeps every bucket in its slots
    newhead = ref_running_max(ref_mark_subheads(ks, al.pos)).astype(U32)
    return keys, ks, al.sac[order], newhead, ref_round_flags(newhead, al.pos)


def same_sets_per_run(keys_sorted, got_vals, want_vals, lo=0, hi=None):
    """values compared as sets per run of equal keys (order among equal keys is not specified)"""
    hi = len(keys_sorted) if hi is None else hi
    c = lo
    while c < hi:
        d = c
        while d + 1 < hi and keys_sorted[d + 1] == keys_sorted[c]:
            d += 1
        if sorted(np.asarray(got_vals[c:d + 1]).tolist()) != sorted(np.asarray(want_vals[c:d + 1]).tolist()):
            return False
        c = d + 1
    return True


# ---------------------------------------------------------------------------------------------------------------------
# reference suffix sort (prefix doubling in numpy) and the inputs of the three call forms
# ---------------------------------------------------------------------------------------------------------------------
def ref_suffix_array(sym, terminator=None):
    """Suffix array of the integer string `sym`; past the end sorts smallest.  terminator: every occurrence of that symbol
    is unique, ordered by position (nothing behind a terminator is ever compared)."""
    sym = np.asarray(sym, dtype=np.int64)
    n = len(sym)
    if n == 0:
        return np.zeros(0, U32)
    if terminator is not None:
        is_t = sym == terminator
        t_count = int(is_t.sum())
        below = sym < terminator
        s2 = np.where(below, sym, sym + t_count)         # room for t_count distinct terminators at the terminator's place
        s2[is_t] = terminator + np.arange(t_count)
        sym = s2
    _, rank = np.unique(sym, return_inverse=True)
    rank = rank.astype(np.int64) + 1
    h = 1
    while True:
        second = np.zeros(n, np.int64)
        if h < n:
            second[:n - h] = rank[h:]
        order = np.lexsort((second, rank))
        r1, r2 = rank[order], second[order]
        new = np.ones(n, np.int64)
        new[1:] = (r1[1:] != r1[:-1]) | (r2[1:] != r2[:-1])
        dense = np.cumsum(new)
        rank = np.empty(n, np.int64)
        rank[order] = dense
        if dense[-1] == n:
            return order.astype(U32)
        h *= 2
        assert h < 4 * n


def naive_suffix_array(sym, terminator=None):
    """sorted() on slices (n <= 2000): the check of ref_suffix_array"""
    s = [int(x) for x in sym]
    if terminator is not None:
        def key(i):
            out = []
            for j in range(i, len(s)):
                if s[j] == terminator:
                    out.append((s[j], j))
                    break
                out.append((s[j], -1))
            return out
        return u32(sorted(range(len(s)), key=key))
    return u32(sorted(range(len(s)), key=lambda i: s[i:]))


def fibonacci_string(n):
    a, b = "b", "a"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def thue_morse(n):
    return "".join("ab"[bin(i).count("1") & 1] for i in range(n))


def text_inputs(n, seed=7):
    """name -> bytes of length n over letters (byte values >= 65)"""
    rng = np.random.default_rng(seed + n)
    out = {
        "a^n": "a" * n,
        "(ab)^n": ("ab" * n)[:n],
        "(abc)^n+x": (("abc" * n)[:max(n - 1, 0)] + "d")[:n],
        "fibonacci": fibonacci_string(n),
        "thue_morse": thue_morse(n),
        "random2": "".join("ac"[x] for x in rng.integers(0, 2, n)),
        "random4": "".join("acgt"[x] for x in rng.integers(0, 4, n)),
    }
    runs = []
    while sum(len(r) for r in runs) < n:
        runs.append("n" * int(rng.integers(50, 5001)) + "acgt"[int(rng.integers(0, 4))])
    out["runs"] = "".join(runs)[:n]
    return {k: np.frombuffer(v.encode(), U8).copy() for k, v in out.items()}


PERIODIC_AND_RUNS = ("a^n", "(ab)^n", "(abc)^n+x", "runs")


def byte_form(text):
    """the engine's call form: dense codes of the bytes that occur, 0 = past the end"""
    hist = np.bincount(text, minlength=256)
    code = np.zeros(256, U8)
    sigma = 0
    for c in range(256):
        if hist[c]:
            sigma += 1
            code[c] = sigma
    bits = max(1, bit_width(sigma))
    return code, bits, min(64 // bits, 64), sigma


def dict_form(text, phrase=997):
    """the dictionary's call form: the text cut into phrases ending in 0x01, the last byte 0x00; both share code 0 with
    the padding and are unique terminators; byte 2 always has a code"""
    t = text.tolist()
    out = []
    for i, x in enumerate(t):
        out.append(x)
        if (i + 1) % phrase == 0:
            out.append(1)
    d = u8(out[:max(len(t) - 1, 0)] + [0]) if len(t) else u8([])
    hist = np.bincount(d, minlength=256)
    code = np.zeros(256, U8)
    sigma = 0
    for c in range(2, 256):
        if hist[c] or c == 2:
            sigma += 1
            code[c] = sigma
    bits = max(1, bit_width(sigma))
    return d, code, bits, min(63 // bits, 63), sigma


def int_form(sym):
    """the parse's call form: symbols 1 .. D, bits = bit_width(D), chars = 64 / bits"""
    d = int(max(sym)) if len(sym) else 1
    bits = max(1, bit_width(d))
    return bits, max(1, 64 // bits)


def round_bound(n, h0):
    """ceil(log2(n / h0)) + 1 rounds at the most (a round with step h orders by 2 h characters; n distinguish all)"""
    r = 0
    while h0 * (1 << r) < n:
        r += 1
    return r + 1


# ---------------------------------------------------------------------------------------------------------------------
# the prefix-free parse: how a text goes to the probe (both layouts of csrc/textref.hpp) and its thin wrappers.
# The references of these kernels are tests/pfpmodel.py.
# ---------------------------------------------------------------------------------------------------------------------
def c_u64(v):
    return ctypes.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


class KpText(ctypes.Structure):
    _fields_ = [("v", ctypes.c_void_p), ("v_len", ctypes.c_uint64), ("misalign", ctypes.c_uint32),
                ("packed", ctypes.c_void_p), ("n_words", ctypes.c_uint64), ("excw", ctypes.c_void_p), ("n_excw", ctypes.c_uint64),
                ("runs", ctypes.c_void_p), ("n_runs", ctypes.c_uint32), ("n", ctypes.c_uint64)]


TX_BLOCK = 4096
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def pack_text(text):
    """The packed layout documented at the top of textref.hpp: (words, excw, runs).  words: 2-bit codes (A C G T -> 0 1 2 3),
    text position p in bits [2 (p & 31), + 2) of word p >> 5, two words of padding; every other byte has code 0 and belongs
    to a run (start, length, byte) -- runs maximal, sorted, disjoint; bit b of excw[b >> 6]: positions [4096 b, + 4096) hold
    part of a run.  runs is an (n_runs, 4) uint32 array: start low, start high, length, byte (the 16-byte record)."""
    text = u8(text); n = len(text)
    words = [0] * ((n + 31) // 32 + 2)
    n_blocks = (n >> 12) + 1
    flags = [0] * ((n_blocks >> 6) + 1)
    runs = []
    for p in range(n):
        b = int(text[p])
        c = _CODE.get(b)
        if c is None:
            if runs and runs[-1][3] == b and runs[-1][0] + runs[-1][2] == p:
                runs[-1][2] += 1
            else:
                runs.append([p, 0, 1, b])
            flags[(p >> 12) >> 6] |= 1 << ((p >> 12) & 63)
        else:
            words[p >> 5] |= c << (2 * (p & 31))
    for r in runs:
        r[0], r[1] = r[0] & 0xFFFFFFFF, r[0] >> 32
    return u64(words), u64(flags), np.array(runs, dtype=U32).reshape(-1, 4)


class Text:
    """a text for the probe.  layout "bytes": V = 0x02 . T . 0x02^32 . zeros (64 bytes of them and more), placed so that
    (v + 1) mod 16 = misalign; layout "packed": the arrays of pack_text"""

    def __init__(self, text, layout="bytes", misalign=0, pad=64):
        self.text = u8(text); self.n = len(self.text); self.layout = layout
        self.v = np.concatenate([np.full(1, 2, U8), self.text, np.full(32, 2, U8), np.zeros(pad, U8)])
        self.c = KpText()
        self.c.n = self.n
        if layout == "bytes":
            self.c.v = self.v.ctypes.data; self.c.v_len = len(self.v); self.c.misalign = misalign
        else:
            assert layout == "packed" and misalign == 0
            self.words, self.excw, self.runs = pack_text(self.text)
            self.c.packed = self.words.ctypes.data; self.c.n_words = len(self.words)
            self.c.excw = self.excw.ctypes.data; self.c.n_excw = len(self.excw)
            self.c.runs = self.runs.ctypes.data if len(self.runs) else None; self.c.n_runs = len(self.runs)

    def arg(self):
        return ctypes.byref(self.c)


def _pos(a, wide):
    return np.ascontiguousarray(a, dtype=U64 if wide else U32)


def _sent_pos(n, wide):
    return np.full(n, SENT64, U64) if wide else np.full(n, SENT32, U32)


def trigger_blocks(n):
    out = np.zeros(1, U32)
    call("trigger_blocks", c_u64(n), out)
    return int(out[0])


def emit_tile():
    out = np.zeros(1, U32)
    call("emit_tile", out)
    return int(out[0])


def trigger_masks(tx, w, p, extra=3):
    """(masks, block_count), both with `extra` sentinel entries behind what the wrapper may write"""
    n = tx.n
    masks = np.full((n + 15) // 16 + extra, 0xA5A5, np.uint16)
    counts = np.full(max(1, ((n + 15) // 16 + 255) // 256) + extra, SENT32, U32)
    call("trigger_masks", tx.arg(), c_u64(n), w, c_u32(p), masks, len(masks), counts, len(counts))
    return masks, counts


def trigger_cuts(masks, n, block_off, alloc, wide):
    cuts = _sent_pos(alloc, wide)
    call("trigger_cuts", np.ascontiguousarray(masks, dtype=np.uint16), c_u64(n), u32(block_off), cuts, alloc, int(wide))
    return cuts


def phrase_bounds(cuts, n, w, wide, extra=2):
    cuts = _pos(cuts, wide); k = len(cuts)
    start = _sent_pos(k + 1 + extra, wide); length = np.full(k + 1 + extra, SENT32, U32)
    call("phrase_bounds", cuts, k, c_u64(n), w, start, length, k + 1 + extra, int(wide))
    return start, length


def phrase_hash(tx, start, length, wide=False, extra=2):
    start = _pos(start, wide); m = len(start)
    h1 = np.full(m + extra, SENT64, U64); pinfo = np.full((m + extra, 4), SENT32, U32)
    call("phrase_hash", tx.arg(), start, u32(length), m, h1, pinfo, m + extra, int(wide))
    return h1, pinfo


def second_fingerprint(pinfo, extra=2):
    pinfo = u32(pinfo).reshape(-1, 4); m = len(pinfo)
    h2 = np.full(m + extra, SENT64, U64)
    call("second_fingerprint", pinfo, m, h2, m + extra)
    return h2


def mark_distinct(order, h1s, pinfo, tx, extra=2):
    order = u32(order); m = len(order); pinfo = u32(pinfo).reshape(-1, 4)
    flags = np.full(m + extra, SENT32, U32); err = np.zeros(16, U32); err[2:] = SENT32
    call("mark_distinct", order, u64(h1s), pinfo, len(pinfo), tx.arg(), m, flags, m + extra, err)
    return flags, err


def assign_distinct(order, scan, flags, length, d_alloc):
    m = len(order)
    pid = np.full(m, SENT32, U32); rep = np.full(d_alloc, SENT32, U32); dlen = np.full(d_alloc, SENT32, U32)
    call("assign_distinct", u32(order), u32(scan), u32(flags), u32(length), m, pid, rep, dlen, d_alloc)
    return pid, rep, dlen


def sum_u32(x):
    x = u32(x); out = np.full(1, SENT64, U64)
    call("sum_u32", x, len(x), out)
    return int(out[0])


def copy_dict(tx, start, length, which, dstart, dict_len, pack_prev, wide=False, with_info=True, extra=8):
    start = _pos(start, wide)
    d = np.full(dict_len + extra, SENT8, U8)
    info = np.full(dict_len + extra, SENT64, U64) if with_info else None
    call("copy_dict", tx.arg(), start, u32(length), len(start), u32(which), u32(dstart), len(which), d, info, dict_len + extra,
         dict_len, int(pack_prev), int(wide))
    return d, info


def entry_info(sa_d, dinfo, d, pack_prev, extra=5):
    nd = len(sa_d)
    esuf = np.full(nd + extra, SENT32, U32); ephr = np.full(nd + extra, SENT32, U32); ebw = np.full(nd + extra, SENT8, U8)
    call("entry_info", u32(sa_d), u64(dinfo), u8(d), nd, int(pack_prev), esuf, ephr, ebw, nd + extra)
    return esuf, ephr, ebw


def dict_irreducible(d, sa_d, esuf, ebw, long_cap, long_alloc):
    nd = len(sa_d)
    plcp = np.full(nd, SENT32, U32); longs = np.full((long_alloc, 4), SENT32, U32); cnt = np.full(1, SENT32, U32)
    call("dict_irreducible", u8(d), nd, u32(sa_d), u32(esuf), u8(ebw), plcp, longs, long_alloc, cnt, long_cap)
    return plcp, longs, int(cnt[0])


def long_lcp_lim(d, longs, plcp):
    longs = u32(longs).reshape(-1, 4); plcp = u32(plcp).copy()
    call("long_lcp_lim", u8(d), len(d), longs, len(longs), plcp)
    return plcp


def plcp_running_max(plcp, extra=3):
    n = len(plcp)
    a = np.concatenate([u32(plcp), np.full(extra, SENT32, U32)])
    call("plcp_running_max", a, n, n + extra)
    return a


def lcp_gather(plcp, sa, extra=5):
    n = len(sa)
    out = np.full(n + extra, SENT32, U32)
    call("lcp_gather", u32(plcp), len(plcp), u32(sa), n, out, n + extra)
    return out


def dict_lcp_clamp(lcp, esuf, extra=3):
    nd = len(esuf)
    a = np.concatenate([u32(lcp)[:nd], np.full(extra, SENT32, U32)])
    call("dict_lcp_clamp", a, u32(esuf), nd, nd + extra)
    return a


def group_flags(esuf, lcp_d, w, extra=2):
    nd = len(esuf)
    g, p, v = (np.full(nd + extra, SENT32, U32) for _ in range(3)); seg = np.full(nd + extra, SENT64, U64)
    call("group_flags", u32(esuf), u32(lcp_d), nd, w, g, p, v, seg, nd + extra)
    return g, p, v, seg


def phrase_ranks(esuf, ephr, pscan, alloc):
    prank = np.full(alloc, SENT32, U32)
    call("phrase_ranks", u32(esuf), u32(ephr), u32(pscan), len(esuf), prank, alloc)
    return prank


def parse_ranks(pid, prank, extra=2):
    m = len(pid); out = np.full(m + extra, SENT32, U32)
    call("parse_ranks", u32(pid), u32(prank), len(prank), m, out, m + extra)
    return out


def invert_ranks(prank, rep, dlen, extra=2):
    d = len(prank)
    which = np.full(d + extra, SENT32, U32); slen = np.full(d + extra, SENT32, U32)
    call("invert_ranks", u32(prank), u32(rep), u32(dlen), d, which, slen, d + extra)
    return which, slen


def occ_sequence(sa_p, pid, n_distinct, extra=2):
    m = len(sa_p)
    keys = np.full(m + 1 + extra, SENT32, U32); vals = np.full(m + 1 + extra, SENT32, U32)
    call("occ_sequence", u32(sa_p), u32(pid), m, c_u32(n_distinct), keys, vals, m + 1 + extra)
    return keys, vals


def occ_finish(mode, ids, ts, sa_p, pstart, wide, sl, pos_bits, n_start, extra=2):
    """mode 8: (occ_start, occ u64, occ_sl); mode 12: (occ_start, occ12 (m + extra, 3), None)"""
    m = len(sa_p)
    occ_start = np.full(n_start, SENT32, U32)
    occ = np.full(m + extra, SENT64, U64) if mode == 8 else np.full((m + extra, 3), SENT32, U32)
    occ_sl = np.full(m + extra, SENT32, U32) if mode == 8 else None
    call("occ_finish", mode, u32(ids), u32(ts), u32(sa_p), _pos(pstart, wide), int(wide), m, occ_start, n_start, occ, m + extra,
         pos_bits, u32(sl), occ_sl)
    return occ_start, occ, occ_sl


def phrase_table(occ_start, plen, rep, extra=2):
    d = len(rep); tab = np.full((d + extra, 4), SENT32, U32)
    call("phrase_table", u32(occ_start), u32(plen), len(plen), u32(rep), d, tab, d + extra)
    return tab


def entry_compact(esuf, ephr, ebw, gflag, gscan, vflag, vscan, seg_min, tab, n_entries, extra=2):
    a = n_entries + extra
    cols = {k: np.full(a, SENT32, U32) for k in ("cnt", "first", "offm1", "gs", "hl", "slen")}
    cols["bwt"] = np.full(a, SENT8, U8)
    tab = u32(tab).reshape(-1, 4)
    call("entry_compact", u32(esuf), u32(ephr), u8(ebw), u32(gflag), u32(gscan), u32(vflag), u32(vscan), u64(seg_min), tab, len(tab),
         len(esuf), a, cols["cnt"], cols["first"], cols["offm1"], cols["bwt"], cols["gs"], cols["hl"], cols["slen"])
    return cols


def group_heads(sege, ce_hl, ce_slen, extra=2):
    g = len(sege); out = np.full((g + extra, 2), SENT32, U32)
    call("group_heads", u32(sege), u32(ce_hl), u32(ce_slen), len(ce_hl), g, out, g + extra)
    return out


def tile_first(segb, tiles, wide, tile_base=0, extra=2):
    segb = _pos(segb, wide)
    out = np.full(tiles - tile_base + 1 + extra, SENT32, U32)
    call("tile_first", segb, len(segb), c_u64(tiles), out, len(out), int(wide), c_u64(tile_base))
    return out


def oversize(segb, wide, extra=2):
    segb = _pos(segb, wide); g = len(segb) - 1
    osize = np.full(g + extra, SENT32, U32); err = np.zeros(16, U32); err[3:] = SENT32
    call("oversize", segb, g, osize, g + extra, err, int(wide))
    return osize, err


def gather_pos(src, idx, wide, extra=2):
    src = _pos(src, wide); out = _sent_pos(len(idx) + extra, wide)
    call("gather_pos", src, len(src), u32(idx), len(idx), out, len(out), int(wide))
    return out


def relative_offsets(fb_off, f0, count, wide, extra=2):
    fb_off = _pos(fb_off, wide); rel = np.full(count + 1 + extra, SENT32, U32)
    call("relative_offsets", fb_off, len(fb_off), f0, count, rel, len(rel), int(wide))
    return rel


def iota(n, extra=3):
    out = np.full(n + extra, SENT32, U32)
    call("iota", out, n, n + extra)
    return out


def gather_u64(src, idx, extra=2):
    out = np.full(len(idx) + extra, SENT64, U64)
    call("gather_u64", u64(src), len(src), u32(idx), len(idx), out, len(out))
    return out


def _rmq_alloc(m):
    nb = (m + 63) // 64
    return nb * (nb.bit_length() + 1) + 8


def build_rmq(vals):
    """(nb, levels, bmin with sentinels behind levels * nb entries)"""
    vals = u32(vals); bmin = np.full(_rmq_alloc(len(vals)), SENT32, U32); dims = np.zeros(2, U32)
    call("build_rmq", vals, len(vals), bmin, len(bmin), dims)
    return int(dims[0]), int(dims[1]), bmin


def rmq_query(vals, pairs):
    """(rmq_min, rmq_min8) of every (a, b)"""
    vals = u32(vals); ab = u32(pairs).reshape(-1, 2)
    out = np.full(len(ab), SENT32, U32); out8 = np.full(len(ab), SENT32, U32)
    call("rmq_query", vals, len(vals), ab, len(ab), out, out8)
    return out, out8


def parse_lcp(tx, nv, sa_p, pid, pstart, wide):
    """ParseLcp::build: (sl, bmin, nb, levels, n_irreducible, n_long)"""
    m = len(sa_p)
    sl = np.full(m, SENT32, U32); bmin = np.full(_rmq_alloc(m), SENT32, U32); dims = np.zeros(4, U32)
    call("parse_lcp", tx.arg(), c_u64(nv), u32(sa_p), u32(pid), _pos(pstart, wide), int(wide), m, sl, bmin, len(bmin), dims)
    return sl, bmin, int(dims[0]), int(dims[1]), int(dims[2]), int(dims[3])


# ---------------------------------------------------------------------------------------------------------------------
# the bucket-wise producer (csrc/guided_kernels.hpp, mmt::gk): gk_<wrapper> calls kp_gk_<wrapper>.  The references are
# tests/guidedmodel.py.  Every in/out array is handed over as the caller made it (sentinels behind what may be written).
# ---------------------------------------------------------------------------------------------------------------------
SENT16 = 0xA5A5


def sent(n, dtype):
    """n sentinel entries of the type"""
    return np.full(n, {1: SENT8, 2: SENT16, 4: SENT32, 8: SENT64}[np.dtype(dtype).itemsize], dtype)


def gk_rank_counts(mask, n_counts, counts):
    mask = u64(mask); call("gk_rank_counts", mask, c_u64(len(mask)), counts, c_u64(n_counts), len(counts))
    return counts


def gk_block_first_cut(mask, n_blocks, first):
    mask = u64(mask); call("gk_block_first_cut", mask, c_u64(len(mask)), first, c_u64(n_blocks), len(first))
    return first


def gk_block_cut_counts(mask, n_blocks, counts):
    mask = u64(mask); call("gk_block_cut_counts", mask, c_u64(len(mask)), counts, c_u64(n_blocks), len(counts))
    return counts


def gk_block_cut_offsets(mask, brank, n_blocks, coff):
    mask = u64(mask); assert coff.dtype == np.uint16
    call("gk_block_cut_offsets", mask, c_u64(len(mask)), u32(brank), coff, c_u64(n_blocks), len(coff))
    return coff


def gk_stage_block_tiles(tile_off, n, blk_tile):
    tile_off = u32(tile_off); call("gk_stage_block_tiles", tile_off, len(tile_off), c_u64(n), blk_tile, len(blk_tile))
    return blk_tile


def gk_stage_count(staged, b0, b1, block_count):
    staged = u32(staged); call("gk_stage_count", staged, c_u64(len(staged)), c_u32(b0), c_u32(b1), block_count, len(block_count))
    return block_count


def gk_heads0(keys, bits, chars, head, active, lcp):
    keys = u64(keys); call("gk_heads0", keys, len(keys), head, active, lcp, len(head), bits, chars)
    return head, active, lcp


def gk_gather_active(idx, pos_sorted, head, slot, pos, headval):
    idx = u32(idx); pos_sorted = u64(pos_sorted)
    call("gk_gather_active", idx, len(idx), pos_sorted, u8(head), len(pos_sorted), slot, pos, headval, len(slot))
    return slot, pos, headval


def gk_medium_groups(ghead, cap, extra=3):
    """(list as (4 * cap + extra, 2) words, count4 with one sentinel word behind it)"""
    ghead = u32(ghead)
    lst = sent((4 * cap + extra) * 2, U32).reshape(-1, 2); cnt = sent(5, U32)
    call("gk_medium_groups", ghead, len(ghead), lst, cap, len(lst), cnt, len(cnt))
    return lst, cnt


def gk_tile_bounds(ghead, target, limit, n_tiles, bound):
    ghead = u32(ghead); call("gk_tile_bounds", ghead, len(ghead), target, c_u32(limit), n_tiles, bound, len(bound))
    return bound


def gk_local_sort(kin, pin, ghead, bound, kout, pout, big_alloc, big_cap):
    kin = u64(kin); m = len(kin)
    bb = sent(big_alloc, U32); be = sent(big_alloc, U32); cnt = np.zeros(1, U32)
    call("gk_local_sort", kin, u64(pin), u32(ghead), m, kout, pout, u32(bound), len(bound) - 1, bb, be, big_alloc, cnt, big_cap)
    return kout, pout, bb, be, int(cnt[0])


def gk_range_groups(ghead, big_begin, big_end, seg_alloc):
    ghead = u32(ghead)
    sb = sent(seg_alloc, U32); se = sent(seg_alloc, U32); cnt = sent(2, U32)
    call("gk_range_groups", ghead, len(ghead), u32(big_begin), u32(big_end), len(big_begin), sb, se, seg_alloc, cnt, len(cnt))
    return sb, se, cnt


def gk_round_apply(pos_sorted, newhead, slot, out, flags):
    newhead = u32(newhead)
    call("gk_round_apply", u64(pos_sorted), newhead, u32(slot), len(newhead), out, len(out), flags, len(flags))
    return out, flags


def gk_round_compact(idx, slot, pos_sorted, newhead, slot_out, pos_out, headval_out):
    idx = u32(idx); slot = u32(slot)
    call("gk_round_compact", idx, len(idx), slot, u64(pos_sorted), u32(newhead), len(slot), slot_out, pos_out, headval_out, len(slot_out))
    return slot_out, pos_out, headval_out


def gk_flag_greater(v, thr, flags):
    v = u32(v); call("gk_flag_greater", v, len(v), c_u32(thr), flags, len(flags))
    return flags


def gk_flag_spread(a, out):
    a = u32(a); call("gk_flag_spread", a, len(a), out, len(out))
    return out


def gk_flag_to_distinct(occ_flag, pid, dflag):
    pid = u32(pid); call("gk_flag_to_distinct", u32(occ_flag), pid, len(pid), dflag, len(dflag))
    return dflag


def gk_flag_from_distinct(dflag, pid, occ_flag):
    dflag = u32(dflag); pid = u32(pid); call("gk_flag_from_distinct", dflag, len(dflag), pid, len(pid), occ_flag, len(occ_flag))
    return occ_flag


def gk_flag_scatter_ones(ids, flags):
    ids = u32(ids); call("gk_flag_scatter_ones", ids, len(ids), flags, len(flags))
    return flags


def gk_giant_distinct(gids, rep, dlen, which, glen):
    gids = u32(gids); rep = u32(rep)
    call("gk_giant_distinct", gids, len(gids), rep, u32(dlen), len(rep), which, glen, len(which))
    return which, glen


def gk_giant_bits(flags, bits):
    flags = u32(flags); call("gk_giant_bits", flags, len(flags), bits, len(bits))
    return bits


def gk_popcount_words(bits, out):
    bits = u32(bits); call("gk_popcount_words", bits, len(bits), out, len(out))
    return out


def gk_giant_map(gids, gstart, dmap):
    gids = u32(gids); call("gk_giant_map", gids, u32(gstart), len(gids), dmap, len(dmap))
    return dmap


def gk_giant_occurrences(gk, pid, pstart, wide, dmap, gps, gbase):
    gk = u32(gk); pid = u32(pid); dmap = u32(dmap)
    call("gk_giant_occurrences", gk, len(gk), pid, _pos(pstart, wide), int(wide), len(pid), dmap, len(dmap), gps, gbase, len(gps))
    return gps, gbase


def gk_giant_group_flags(esuf, lcp, flags):
    esuf = u32(esuf); call("gk_giant_group_flags", esuf, u32(lcp), len(esuf), flags, len(flags))
    return flags


def gk_group_ids(ce_gs, gscan, B):
    call("gk_group_ids", ce_gs, u32(gscan), B, len(ce_gs))
    return ce_gs


def gk_add_offset(table, n, add):
    call("gk_add_offset", table, int(table.itemsize == 8), n, c_u64(add), len(table))
    return table


def gk_rep_bits(pid, rep, bits):
    pid = u32(pid); rep = u32(rep); call("gk_rep_bits", pid, rep, len(rep), len(pid), bits, len(bits))
    return bits


class KpCtx(ctypes.Structure):
    _fields_ = [("T", ctypes.c_void_p), ("n", ctypes.c_uint64), ("w", ctypes.c_uint32),
                ("mask", ctypes.c_void_p), ("n_mask", ctypes.c_uint64), ("rdir", ctypes.c_void_p), ("n_rdir", ctypes.c_uint64),
                ("nxt", ctypes.c_void_p), ("n_nxt", ctypes.c_uint64),
                ("isa_p", ctypes.c_void_p), ("m", ctypes.c_uint32), ("code", ctypes.c_void_p), ("bits", ctypes.c_int), ("chars", ctypes.c_int),
                ("skip", ctypes.c_uint32), ("pos_bits", ctypes.c_uint32), ("rec_rank", ctypes.c_uint32), ("no_dense", ctypes.c_uint32),
                ("pid", ctypes.c_void_p), ("coff", ctypes.c_void_p), ("n_coff", ctypes.c_uint64), ("brank", ctypes.c_void_p), ("n_brank", ctypes.c_uint64),
                ("g_k", ctypes.c_void_p), ("g_ps", ctypes.c_void_p), ("g_base", ctypes.c_void_p), ("g_n", ctypes.c_uint32),
                ("g_isa", ctypes.c_void_p), ("g_grp", ctypes.c_void_p), ("g_lcp", ctypes.c_void_p), ("n_gisa", ctypes.c_uint32),
                ("g_depth", ctypes.c_uint32), ("g_bits", ctypes.c_void_p), ("g_rank", ctypes.c_void_p), ("repbits", ctypes.c_void_p),
                ("n_bitwords", ctypes.c_uint32), ("expand", ctypes.c_uint32)]


class KpRunSlice(ctypes.Structure):
    _fields_ = [("sym", ctypes.c_uint32), ("blo", ctypes.c_uint32), ("bhi", ctypes.c_uint32), ("lead", ctypes.c_void_p),
                ("first", ctypes.c_void_p), ("follow", ctypes.c_void_p), ("n_tiles", ctypes.c_uint64)]


class GkCtx:
    """gk::Ctx for the probe from a model context (tests/guidedmodel.py Ctx): the text in `text_layout` ("bytes" / "packed"),
    the phrase ends as "bits" (mask, rdir) or as "list" (coff, brank).  Keeps every array alive."""

    def __init__(self, c, text_layout="bytes", cuts="bits", no_dense=0):
        self.tx = Text(c.text, text_layout)
        t = c.t
        self.keep = {"nxt": u64(t.nxt), "code": u8(c.code)}
        if cuts == "bits":
            self.keep.update(mask=u64(t.mask), rdir=u32(np.concatenate([t.rdir, [0]])))
        else:
            assert cuts == "list"
            self.keep.update(coff=np.ascontiguousarray(t.coff, dtype=np.uint16), brank=u32(t.brank))
        for name in ("isa_p", "pid"):
            if getattr(c, name) is not None:
                self.keep[name] = u32(getattr(c, name))
        if c.rep is not None:
            self.keep["repbits"] = c.bitwords(c.rep)
        g = c.giant
        if g is not None:
            bits = c.bitwords(g.flag)
            self.keep.update(g_k=u32(g.k), g_ps=u64(g.ps), g_base=u32(g.base), g_isa=u32(g.isa), g_grp=u32(g.grp), g_lcp=u32(g.lcp),
                             g_bits=bits, g_rank=g.rank_words(bits))
        k = self.k = KpCtx()
        k.T = ctypes.addressof(self.tx.c); k.n = c.n; k.w = c.w; k.m = c.m; k.bits = c.bits; k.chars = c.chars
        k.skip = c.skip; k.pos_bits = c.pos_bits; k.rec_rank = c.rec_rank; k.no_dense = no_dense; k.expand = c.expand
        k.g_depth = c.g_depth; k.g_n = 0 if g is None else len(g.k); k.n_gisa = 0 if g is None else len(g.isa)
        k.n_bitwords = c.m // 32 + 1
        for name, a in self.keep.items():
            setattr(k, name, a.ctypes.data)
            if hasattr(k, "n_" + name):
                setattr(k, "n_" + name, len(a))

    def arg(self):
        return ctypes.byref(self.k)


def run_slice_arg(rs):
    """(ctypes argument, what keeps it alive) of a model RunSlice, or (NULL, None)"""
    if rs is None:
        return None, None
    keep = (u64(rs.lead), u8(rs.first), u8(rs.follow))
    r = KpRunSlice(rs.sym, rs.blo, rs.bhi, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, len(keep[0]))
    return ctypes.byref(r), (r, keep)


def gk_tile_lead(g, first, lead, follow):
    call("gk_tile_lead", g.arg(), first, lead, follow, len(first))
    return first, lead, follow


def gk_run_hist(g, pc, bin_, rs, hist):
    a, keep = run_slice_arg(rs)
    call("gk_run_hist", g.arg(), pc, c_u32(bin_), a, hist, len(hist))
    return hist


def gk_bin_hist(g, pc, hist):
    call("gk_bin_hist", g.arg(), pc, hist, len(hist))
    return hist


def gk_batch_count(g, pc, lo, hi, tile_count, rs=None):
    a, keep = run_slice_arg(rs)
    call("gk_batch_count", g.arg(), pc, c_u32(lo), c_u32(hi), a, tile_count, len(tile_count))
    return tile_count


def gk_batch_fill(g, pc, lo, hi, tile_off, keys, pos, next_lo, next_hi, next_count, rs=None):
    a, keep = run_slice_arg(rs)
    call("gk_batch_fill", g.arg(), pc, c_u32(lo), c_u32(hi), u32(tile_off), keys, pos, len(keys), c_u32(next_lo), c_u32(next_hi),
         next_count, 0 if next_count is None else len(next_count), a)
    return keys, pos, next_count


def gk_stage_fill(g, pc, lo, hi, tile_off, staged, next_lo, next_hi, next_count):
    call("gk_stage_fill", g.arg(), pc, c_u32(lo), c_u32(hi), u32(tile_off), staged, len(staged), c_u32(next_lo), c_u32(next_hi),
         next_count, 0 if next_count is None else len(next_count))
    return staged, next_count


def gk_stage_take(g, staged, b0, b1, block_off, keys, pos, nb0, nb1, next_count, tile_off, blk_tile):
    staged = u32(staged)
    call("gk_stage_take", g.arg(), staged, c_u64(len(staged)), c_u32(b0), c_u32(b1), u32(block_off), keys, pos, len(keys), c_u32(nb0),
         c_u32(nb1), next_count, 0 if next_count is None else len(next_count), u32(tile_off), u32(blk_tile))
    return keys, pos, next_count


def gk_phrase_items(g, pstart, wide, rep, keys, pos):
    pstart = _pos(pstart, wide); rep = u32(rep)
    call("gk_phrase_items", g.arg(), pstart, int(wide), len(pstart), rep, len(rep), keys, pos, len(keys))
    return keys, pos


def gk_round_keys(g, pos, offset, keys, err, gr=None, pure=None, ghead=None):
    pos = u64(pos)
    call("gk_round_keys", g.arg(), pos, len(pos), c_u64(offset), keys, len(keys), err, None if gr is None else u32(gr),
         None if pure is None else u8(pure), None if ghead is None else u32(ghead))
    return keys, err


def gk_giant_probe(g, pos, ghead, offset, gr, pure):
    pos = u64(pos)
    call("gk_giant_probe", g.arg(), pos, u32(ghead), len(pos), c_u64(offset), gr, pure, len(gr))
    return gr, pure


def gk_round_heads(g, keys, ghead, headval, err, lcp_out=None, slot=None, offset=0, pure=None):
    keys = u64(keys)
    call("gk_round_heads", g.arg(), keys, u32(ghead), len(keys), headval, len(headval), err, lcp_out,
         0 if lcp_out is None else len(lcp_out), None if slot is None else u32(slot), c_u64(offset), None if pure is None else u8(pure))
    return headval, err, lcp_out


def gk_write_columns(g, pos, base, sa_lo, sa_hi, bwt):
    pos = u64(pos)
    call("gk_write_columns", g.arg(), pos, len(pos), c_u64(base), sa_lo, sa_hi, bwt, len(sa_lo))
    return sa_lo, sa_hi, bwt


def gk_phrase_ranks(g, pos, pid, prank):
    pos = u64(pos)
    call("gk_phrase_ranks", g.arg(), pos, len(pos), u32(pid), prank, len(prank))
    return prank


def gk_expand_entries(g, pos, lcp, tab, cols, err):
    pos = u64(pos); tab = u32(tab).reshape(-1, 4)
    call("gk_expand_entries", g.arg(), pos, u32(lcp), len(pos), tab, len(tab), cols["cnt"], cols["first"], cols["offm1"], cols["bwt"],
         cols["gs"], cols["hl"], cols["slen"], len(cols["cnt"]), err)
    return cols, err


def gk_resolve_small(g, pos, ghead, slot, offset, out, flags, err, lcp_out=None, limit=0):
    pos = u64(pos)
    call("gk_resolve_small", g.arg(), pos, u32(ghead), u32(slot), len(pos), c_u64(offset), out, len(out), flags, len(flags), err, lcp_out, limit)
    return out, flags, err, lcp_out


def gk_batch_lcp(g, sl, pos, carry, lcp, err):
    pos = u64(pos); sl = u32(sl)
    call("gk_batch_lcp", g.arg(), sl, len(sl), pos, len(pos), None if carry is None else u64(carry), lcp, len(lcp), err)
    return lcp, err


def gk_resolve_medium(g, sl, pos, slot, classes, cap, offset, out, flags, err, lcp_out=None):
    """classes: four lists of (first, size); laid out as the four regions of `cap` pairs"""
    pos = u64(pos); sl = u32(sl)
    lst = sent(8 * cap, U32).reshape(4, cap, 2)
    for cl, groups in enumerate(classes):
        for i, (first, size) in enumerate(groups):
            lst[cl, i] = (first, size)
    n_groups = u32([len(x) for x in classes])
    call("gk_resolve_medium", g.arg(), sl, len(sl), pos, len(pos), u32(slot), lst, cap, n_groups, c_u64(offset), out, len(out), flags,
         len(flags), lcp_out, err)
    return out, flags, err, lcp_out
