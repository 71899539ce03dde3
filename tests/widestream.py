"""Synthetic wide streams: the oracle stream of a small real collection, moved onto a virtual text of up to 2^39
characters, so that the 40-bit paths run with real 40-bit values in milliseconds.

Every document d gets a virtual pad of pre[d] characters before its bases and post[d] after them: document d becomes
pad F_d pad '$' [revcomp '$'] with L'_d = L_d + pre[d] + post[d].  A pad before the bases raises the document's
in-document offsets; a pad after them moves the absolute positions of every later document (and, under revcomp, the
rc copy of the document itself).  Each entry keeps its order, LCP, BWT byte, document and strand; only its suffix-array
position moves.  The pads are never materialised: the stream is a prefix of a stream over the virtual text (the
entries of the real suffixes of the small collection), which the engine, the CLI's -a reader and both host checkers
accept."""
import numpy as np

import pyoracle as O

G32 = 1 << 32
G33 = 1 << 33
G39 = 1 << 39


def small_stream(docs, revcomp):
    """(sa, lcp, bwt) of the real suffixes (sentinel entry dropped) and the per-document base counts."""
    text, _ = O.build_text(docs, revcomp)
    sa, lcp, bwt = O.build_stream(text)
    return sa[1:].copy(), lcp[1:].copy(), bwt[1:].copy(), [sum(len(r) for r in d) for d in docs]


def pad_stream(sa, doc_bases, revcomp, pads):
    """sa of the small text -> (sa on the virtual text, per-document text lengths of the virtual text)."""
    k = 2 if revcomp else 1
    L = np.asarray(doc_bases, np.int64)
    pre = np.array([p[0] for p in pads], np.int64)
    post = np.array([p[1] for p in pads], np.int64)
    Lp = L + pre + post
    start = np.zeros(len(L) + 1, np.int64)
    start[1:] = np.cumsum(k * (L + 1))
    startp = np.zeros(len(L) + 1, np.int64)
    startp[1:] = np.cumsum(k * (Lp + 1))
    sa = np.asarray(sa, np.int64)
    d = np.searchsorted(start, sa, side="right") - 1
    r = sa - start[d]
    half = L[d] + 1
    halfp = Lp[d] + 1
    fwd = r < half
    q = r - half
    rp = np.where(fwd, np.where(r < L[d], r + pre[d], Lp[d]),               # forward bases / its '$'
                  np.where(q < L[d], halfp + post[d] + q, 2 * halfp - 1))   # rc(pad_post) rc(F) rc(pad_pre) / '$'
    return startp[d] + rp, (k * (Lp + 1)).tolist()


def schedule(n_docs, doc_bases, revcomp, where="both", top=G39 - 4099):
    """Pads that put document starts and entries across 2^32, 2^33 and up to `top` (< 2^40), with one document longer
    than 2^32 characters.  Document 0 is never padded (merge metadata is sized by it).  where: "pre" (before the bases
    only), "post" (after them only) or "both"."""
    k = 2 if revcomp else 1
    big = [G32 + 977, G33 + 1, 3000000019, G32 - 5]
    pads = [[0, 0] for _ in range(n_docs)]
    for d in range(1, n_docs - 1):
        side = {"pre": 0, "post": 1}.get(where, d % 2)
        pads[d][side] = big[d - 1] if d <= len(big) else 1000003 * d      # (many documents: the rest small)
    if n_docs >= 2:
        used = sum(k * (doc_bases[d] + pads[d][0] + pads[d][1] + 1) for d in range(n_docs - 1))
        last_len = (top - used) // k - 1                # L' of the last document, its text ending just below `top`
        fill = last_len - doc_bases[-1]
        assert fill > G32, "collection too large for the schedule"
        pads[-1][0 if where == "pre" else 1] = fill
    return pads


def wide(docs, revcomp, where="both", top=G39 - 4099):
    """docs -> (sa, lcp, bwt, virtual per-document text lengths, pads, small-text per-document text lengths)."""
    sa, lcp, bwt, bases = small_stream(docs, revcomp)
    pads = schedule(len(docs), bases, revcomp, where, top)
    sap, lens = pad_stream(sa, bases, revcomp, pads)
    k = 2 if revcomp else 1
    return sap, lcp, bwt, lens, pads, [k * (b + 1) for b in bases]


def expected_rows(rows, pads, bases, revcomp, mummode):
    """The metamorphic relation where it is exact: revcomp off with pads before the bases (offset + pre), revcomp on
    with pads after the bases ('+' offsets unchanged but the terminator's, '-' offsets unchanged).  rows = oracle
    mum_rows() or mem_rows() of the small stream; returns the rows expected of the padded one."""
    pre = np.array([p[0] for p in pads], np.int64)
    post = np.array([p[1] for p in pads], np.int64)
    L = np.asarray(bases, np.int64)
    if mummode:
        length, off, st = rows
        off = off.copy()
        d = np.broadcast_to(np.arange(off.shape[1]), off.shape)
        plus = (st == 1) & (off >= 0)
        if not revcomp:
            assert not post.any()
            off[plus] += pre[d[plus]]
        else:
            assert not pre.any()
            term = plus & (off == L[d])
            off[term] += post[d[term]]
        return length, off, st
    length, occ, off, docs, st = rows
    off = off.copy()
    plus = st == 1
    if not revcomp:
        assert not post.any()
        off[plus] += pre[docs[plus]]
    else:
        assert not pre.any()
        term = plus & (off == L[docs])
        off[term] += post[docs[term]]
    return length, occ, off, docs, st
