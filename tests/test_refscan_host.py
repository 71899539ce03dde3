"""CPU: the C restatement of the match scan and its writers (oracle/mumemto_oracle.c) against the reference's own
mem_finder.hpp (oracle/_ref/mem_finder_ref, tests/refscan.py), byte for byte, on the same streams.  Every GPU
byte-parity test compares with the restatement, so this pins the whole chain to the reference's scan, writers and
merge thresholds: .mums / .mems / .bumbl, .thresh / .thresh_rev and .athresh.

Streams: the oracle stream of each collection (the real suffixes, sentinel entry dropped), and the same streams moved
onto virtual texts of up to 2^39 characters (tests/widestream.py) for the 40-bit arithmetic."""
import numpy as np
import pytest

import refscan as R
import widestream as W
from fuzz_run import adversarial
from mumemto_amd import synth
from test_gpu_random import random_collection, random_params

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/mem_finder_ref not built (needs the reference "
                                                          "tree at build time)")


def modes(n_docs):
    """strict, -k, -f, -F and MEM mode: (name, scan params, flags) with flags a subset of binary / merge / anchor."""
    k = max(2, n_docs - 1)
    return [("strict", dict(num_distinct=n_docs, max_doc_freq=1, max_total_freq=0), ()),
           ("strict-merge", dict(num_distinct=n_docs, max_doc_freq=1, max_total_freq=0), ("merge",)),
           ("strict-anchor", dict(num_distinct=n_docs, max_doc_freq=1, max_total_freq=0), ("merge", "anchor")),
           ("strict-binary", dict(num_distinct=n_docs, max_doc_freq=1, max_total_freq=0), ("binary",)),
           ("k", dict(num_distinct=k, max_doc_freq=1, max_total_freq=0), ()),
           ("f", dict(num_distinct=k, max_doc_freq=2, max_total_freq=0), ()),
           ("F", dict(num_distinct=2, max_doc_freq=0, max_total_freq=2 * n_docs), ()),
           ("mem", dict(num_distinct=2, max_doc_freq=0, max_total_freq=0), ())]


def compare(tmp_path, sa, lcp, bwt, lens, min_len, params, flags, revcomp, tag="c"):
    """Both checkers on one stream; asserts equal files and returns them (None when the reference refuses: .bumbl
    without any MUM, see oracle/_ref_drivers/mem_finder_driver.cpp)."""
    binary, merge, anchor = "binary" in flags, "merge" in flags, "anchor" in flags
    res = R.oracle_result(sa, lcp, bwt, lens, min_len=min_len, revcomp=revcomp, merge=merge, **params)
    want = R.oracle_files(res, lens, revcomp, binary, merge, anchor)
    if binary and res.mum_rows()[0].size == 0:
        return None
    got = R.run(sa, lcp, bwt, lens, tmp_path, min_len=min_len, revcomp=revcomp, binary=binary, merge=merge,
                anchor_merge=anchor, tag=tag, **params)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for ext in want:
        assert got[ext] == want[ext], "%s differs (%d vs %d bytes), params %s flags %s revcomp %s" % (
            ext, len(got[ext]), len(want[ext]), params, flags, revcomp)
    return want


def sweep(tmp_path, docs, min_len, revcomp, which=None):
    sa, lcp, bwt, _ = W.small_stream(docs, revcomp)
    lens = R.doc_text_lengths(docs, revcomp)
    n = 0
    for name, params, flags in modes(len(docs)):
        if which is None or name in which:
            n += compare(tmp_path, sa, lcp, bwt, lens, min_len, params, flags, revcomp) is not None
    return n


@pytest.mark.parametrize("seed", range(6))
def test_random_collections_every_mode(tmp_path, seed):
    """test_gpu_random's generator (IUPAC R/Y/N, lowercase, multi-record documents, inversions, tandem copies, homopolymer
    runs) with its random parameters, and every mode on each collection."""
    rng = np.random.default_rng(5100 + seed)
    n = 0
    for case in range(25):
        docs = random_collection(rng)
        revcomp = bool(case % 2)
        p = random_params(rng, len(docs))
        min_len = p.pop("min_len")
        merge = p["max_doc_freq"] == 1 and p["num_distinct"] == len(docs) and bool(rng.integers(0, 2))
        sa, lcp, bwt, _ = W.small_stream(docs, revcomp)
        lens = R.doc_text_lengths(docs, revcomp)
        n += compare(tmp_path, sa, lcp, bwt, lens, min_len, p, ("merge",) if merge else (), revcomp) is not None
        n += sweep(tmp_path, docs, int(rng.integers(3, 16)), revcomp)
    assert n >= 150


@pytest.mark.parametrize("seed", [7706, 7707, 7711])
def test_adversarial_collections(tmp_path, seed):
    """fuzz_run.py adv: runs of N / of one base up to 12 kbp, tandem arrays, exact copies, large deletions.  (Seeds whose
    reference scan takes seconds, not minutes: its check_doc_range is quadratic in nested intervals of long runs.)"""
    rng = np.random.default_rng(seed)
    for case in range(3):
        docs = adversarial(rng)
        sweep(tmp_path, docs, int(rng.choice([10, 20, 31])), bool((seed + case) % 2),
              which=("strict", "strict-merge", "strict-anchor", "f", "mem"))


def test_iupac_lowercase_multirecord(tmp_path):
    rng = np.random.default_rng(91)
    base = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 4000))
    iupac = b"RYKMSWBDHVN"
    docs = []
    for d in range(5):
        s = bytearray(base)
        for _ in range(60):
            s[int(rng.integers(0, len(s)))] = iupac[int(rng.integers(0, len(iupac)))]
        s[100 * d:100 * d + 300] = s[100 * d:100 * d + 300].lower()
        s[2000:2000 + 50 * d] = b"N" * (50 * d)
        cut = int(rng.integers(1, len(s)))
        docs.append([bytes(s[:cut]), bytes(s[cut:])])
    for revcomp in (True, False):
        assert sweep(tmp_path, docs, 12, revcomp) >= 7


@pytest.mark.parametrize("n_docs", [65, 97, 128])
def test_many_documents(tmp_path, n_docs):
    docs = synth.pangenome(n_docs, 1200, 0.02, seed=n_docs, inversion=(3, 100, 300))
    sweep(tmp_path, docs, 15, n_docs % 2 == 1)


def test_six_thousand_documents(tmp_path):
    rng = np.random.default_rng(6000)
    core = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60))
    docs = []
    for d in range(6000):
        s = bytearray(core)
        s[int(rng.integers(0, 60))] = b"ACGT"[d % 4]
        docs.append([bytes(s[: 40 + d % 20])])
    for revcomp in (True, False):
        sweep(tmp_path, docs, 12, revcomp, which=("strict", "strict-merge", "k", "mem"))


def test_matches_over_65535_saturate_the_thresholds(tmp_path):
    """A 70 kbp identical stretch: MUM lengths above 65,535, the u16 thresholds capped."""
    rng = np.random.default_rng(70)
    stretch = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 70000))
    docs = []
    for d in range(3):
        flank = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 500 + 100 * d))
        docs.append([flank + stretch + flank[::-1]])
    docs[2] = [docs[2][0] + stretch[:68000]]                 # a second, shorter copy: the next best match is over 65,535
    for revcomp in (True, False):
        sa, lcp, bwt, _ = W.small_stream(docs, revcomp)
        lens = R.doc_text_lengths(docs, revcomp)
        want = compare(tmp_path, sa, lcp, bwt, lens, 20, dict(num_distinct=3, max_doc_freq=1, max_total_freq=0),
                       ("merge",), revcomp)
        assert int(want[".mums"].split(b"\t")[0]) > 65535
        th = np.frombuffer(want[".thresh"], np.uint16)
        assert (th == 65535).any()
        compare(tmp_path, sa, lcp, bwt, lens, 20, dict(num_distinct=3, max_doc_freq=1, max_total_freq=0),
                ("merge", "anchor"), revcomp)
        compare(tmp_path, sa, lcp, bwt, lens, 20, dict(num_distinct=2, max_doc_freq=0, max_total_freq=0), (), revcomp)


# ---- wide streams (tests/widestream.py) -----------------------------------------------------------------------------

WIDE_DOCS = [("pangenome", lambda: synth.pangenome(5, 3000, 0.01, seed=7, inversion=(2, 500, 900))),
             ("random", lambda: random_collection(np.random.default_rng(424242))),
             ("many", lambda: synth.pangenome(70, 300, 0.03, seed=70))]


@pytest.mark.parametrize("name,make", WIDE_DOCS, ids=[w[0] for w in WIDE_DOCS])
@pytest.mark.parametrize("where", ["both", "pre", "post"])
@pytest.mark.parametrize("revcomp", [True, False])
def test_wide_stream_both_checkers_agree(tmp_path, name, make, where, revcomp):
    """Entries, document starts and in-document offsets beyond 2^32, 2^33 and up to 2^39 - 4099; one document longer
    than 2^32 characters; the '-' strand arithmetic with half >= 2^32."""
    docs = make()
    if len(docs) < 3:
        docs = docs + docs[:1]
    sa, lcp, bwt, lens, pads, _ = W.wide(docs, revcomp, where)
    assert sa.max() >= W.G39 - (1 << 20) and max(lens) > 2 * W.G32 and sa.max() < 1 << 40
    n_wide = 0
    for mname, params, flags in modes(len(docs)):
        want = compare(tmp_path, sa, lcp, bwt, lens, 12, params, flags, revcomp, tag=mname)
        if want and (".mums" in want or ".mems" in want):
            txt = want.get(".mums", want.get(".mems"))
            n_wide += any(len(x) >= 10 for x in txt.replace(b"\t", b",").replace(b"\n", b",").split(b","))
    if where != "post":
        assert n_wide > 0, "no field of 10 digits or more: the pads did not reach the rows"


def test_wide_stream_mem_mode_wraps_write_mem(tmp_path):
    """MEM mode, revcomp: an occurrence that runs into the terminator of its rc copy makes write_mem's size_t
    arithmetic wrap (mem_finder.hpp:222-227, 244-247) -- a 20-digit position -- on a 40-bit stream too."""
    docs = synth.pangenome(5, 3000, 0.01, seed=7, inversion=(2, 500, 900))
    sa, lcp, bwt, lens, pads, _ = W.wide(docs, True, "both")
    want = compare(tmp_path, sa, lcp, bwt, lens, 12, dict(num_distinct=2, max_doc_freq=0, max_total_freq=0), (), True)
    fields = want[".mems"].replace(b"\t", b",").replace(b"\n", b",").split(b",")
    assert any(len(f) == 20 and int(f) >= 1 << 63 for f in fields)


@pytest.mark.parametrize("revcomp,where", [(False, "pre"), (True, "post")])
@pytest.mark.parametrize("mode", ["strict", "k", "f", "mem"])
def test_wide_stream_metamorphic(tmp_path, revcomp, where, mode):
    """Where the relation is exact: revcomp off with pads before the bases (offset + pre), revcomp on with pads after
    them (offsets unchanged, but the forward terminator).  Also: the merge thresholds of an unpadded document 0."""
    docs = synth.pangenome(6, 2500, 0.01, seed=11, inversion=(3, 400, 800))
    params = {name: p for name, p, _ in modes(len(docs))}[mode]
    sa0, lcp0, bwt0, bases = W.small_stream(docs, revcomp)
    lens0 = R.doc_text_lengths(docs, revcomp)
    sa, lcp, bwt, lens, pads, _ = W.wide(docs, revcomp, where)
    small = R.oracle_result(sa0, lcp0, bwt0, lens0, min_len=12, revcomp=revcomp, merge=mode == "strict", **params)
    big = R.oracle_result(sa, lcp, bwt, lens, min_len=12, revcomp=revcomp, merge=mode == "strict", **params)
    mum = params["max_doc_freq"] == 1
    rows_small = small.mum_rows() if mum else small.mem_rows()
    rows_big = big.mum_rows() if mum else big.mem_rows()
    exp = W.expected_rows(rows_small, pads, bases, revcomp, mum)
    assert len(exp[0]) > 0
    for a, b in zip(exp, rows_big):
        assert np.array_equal(a, b)
    if mode == "strict":
        assert np.array_equal(small.thresh_file(False), big.thresh_file(False))
        assert np.array_equal(small.thresh_file(True), big.thresh_file(True))
    compare(tmp_path, sa, lcp, bwt, lens, 12, params, ("merge",) if mode == "strict" else (), revcomp)
