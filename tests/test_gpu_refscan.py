"""GPU against the reference's own match scan (oracle/_ref/mem_finder_ref, tests/refscan.py):
  * wide streams (tests/widestream.py): real 40-bit suffix-array entries, document starts and in-document offsets
    beyond 2^32 / 2^33 up to 2^39, fed through Engine.set_stream40 in every mode -- .mums / .mems, rows, thresholds
    and .bumbl equal the reference's bytes; again under MMT_SCAN_RANGE=8192 / MMT_SCAN_WIDE_AT=2 and with 70 documents;
  * the CLI's 40-bit -a reader end to end on the same files;
  * the GPU's own stream of small collections (every producer, and the packed text) through the reference scan;
  * one 94 x 256 kbp collection (~48 M entries) without the C oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE]
import refscan as R                                   # noqa: E402
import widestream as W                                # noqa: E402
from mumemto_amd import synth                         # noqa: E402
from test_gpu_random import random_collection         # noqa: E402

pytestmark = pytest.mark.gpu
need_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref/mem_finder_ref not built (needs the reference tree "
                                                        "at build time)")

MODES = [("strict", dict(max_doc_freq=1), ()), ("strict-merge", dict(max_doc_freq=1), ("merge",)),
         ("strict-binary", dict(max_doc_freq=1), ("binary",)), ("k", dict(max_doc_freq=1, num_distinct=3), ()),
         ("f", dict(max_doc_freq=2, num_distinct=3), ()), ("F", dict(max_doc_freq=0, num_distinct=2, max_total_freq=8), ()),
         ("mem", dict(max_doc_freq=0, num_distinct=2), ())]


def collections():
    return [("pangenome", synth.pangenome(5, 3000, 0.01, seed=7, inversion=(2, 500, 900))),
            ("random", random_collection(np.random.default_rng(424242)) * 2),
            ("many", synth.pangenome(70, 300, 0.03, seed=70))]


def check_wide(eng, workdir, which=("pangenome", "random", "many"), wheres=("both", "pre", "post")):
    """Every wide stream x mode through the engine; returns the number of runs compared."""
    n = 0
    for name, docs in collections():
        if name not in which:
            continue
        for revcomp in (True, False):
            for where in wheres:
                sa, lcp, bwt, lens, pads, _ = W.wide(docs, revcomp, where)
                bases = [sum(len(r) for r in d) + p[0] + p[1] for d, p in zip(docs, pads)]
                eng.set_stream40(sa, lcp, bwt, bases, use_revcomp=revcomp)
                for mname, params, flags in MODES:
                    p = dict(num_distinct=len(docs), max_total_freq=0)
                    p.update(params)
                    merge, binary = "merge" in flags, "binary" in flags
                    res = R.oracle_result(sa, lcp, bwt, lens, min_len=12, revcomp=revcomp, merge=merge, **p)
                    if binary and res.mum_rows()[0].size == 0:
                        continue
                    ref = R.run(sa, lcp, bwt, lens, workdir, min_len=12, revcomp=revcomp, binary=binary, merge=merge,
                                anchor_merge=merge, tag=mname, **p)
                    eng.run(min_match_len=12, num_distinct=p["num_distinct"], max_doc_freq=p["max_doc_freq"],
                            max_total_freq=p["max_total_freq"], use_revcomp=revcomp, merge_metadata=merge)
                    where_s = "%s %s revcomp=%s %s" % (name, where, revcomp, mname)
                    if binary:
                        assert eng.output_bumbl() == ref[".bumbl"], where_s
                    else:
                        assert eng.output_text() == ref[".mums" if p["max_doc_freq"] == 1 else ".mems"], where_s
                    if p["max_doc_freq"] == 1:
                        for a, b in zip(eng.rows_mum(), res.mum_rows()):
                            assert np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64)), where_s
                    else:
                        for a, b in zip(eng.rows_mem(), res.mem_rows()):
                            assert np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64)), where_s
                    if merge:
                        th = eng.thresholds()
                        assert th[: lens[0] // (2 if revcomp else 1)].tobytes() == ref[".athresh"], where_s
                        assert np.array_equal(th, res.thresh()), where_s
                    n += 1
    return n


@need_ref
def test_wide_streams_every_mode(tmp_path):
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    try:
        assert check_wide(eng, tmp_path) >= 100
    finally:
        eng.close()


@need_ref
@pytest.mark.parametrize("env", [{"MMT_SCAN_RANGE": "8192"}, {"MMT_SCAN_WIDE_AT": "2"}], ids=["range8192", "wide_at2"])
def test_wide_streams_scan_variants(tmp_path, env):
    """The windowed scan (MMT_SCAN_RANGE) and the wide-interval path of k_scan (MMT_SCAN_WIDE_AT, read once per process):
    in a fresh process."""
    r = subprocess.run([sys.executable, __file__, str(tmp_path)], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "wide ok" in r.stdout


def _write_cli_arrays(prefix, sa, lcp, bwt, docs, pads, text_chars):
    """The -a files of a stream prefix: the sentinel entry (sa = |T|) then the real suffixes, and PREFIX.lengths."""
    R.write_arrays(prefix, np.concatenate([[text_chars], sa]), np.concatenate([[0], lcp]),
                   np.concatenate([[ord("$")], bwt]).astype(np.uint8), [])
    with open(prefix + ".lengths", "w") as f:
        for i, (d, p) in enumerate(zip(docs, pads)):
            f.write("/data/d%d.fa * %d\n" % (i, sum(len(r) for r in d) + p[0] + p[1]))


@need_ref
def test_cli_arrays_in_wide_stream(tmp_path):
    """mumemto_exec -a on a 40-bit stream prefix over a virtual text of ~2^39 characters: the CLI's 40-bit reader end
    to end, against the reference scan of the same real suffixes."""
    from mumemto_amd import build
    exe = os.path.join(os.path.dirname(build.LIB), "..", "bin", "mumemto_exec")
    docs = synth.pangenome(5, 3000, 0.01, seed=7, inversion=(2, 500, 900))
    for revcomp in (True, False):
        sa, lcp, bwt, lens, pads, _ = W.wide(docs, revcomp, "both")
        pre = str(tmp_path / ("arr%d" % revcomp))
        _write_cli_arrays(pre, sa, lcp, bwt, docs, pads, sum(lens))
        for flags, p in [([], dict(max_doc_freq=1)), (["-f", "0", "-k", "2"], dict(max_doc_freq=0, num_distinct=2))]:
            q = dict(num_distinct=len(docs), max_total_freq=0)
            q.update(p)
            out = str(tmp_path / ("out%d%d" % (revcomp, len(flags))))
            args = [exe, "-a", pre, "-o", out, "-l", "12"] + flags + ([] if revcomp else ["-r"])
            r = subprocess.run(args, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr[-2000:]
            ref = R.run(sa, lcp, bwt, lens, tmp_path, min_len=12, revcomp=revcomp, **q)
            ext = ".mums" if q["max_doc_freq"] == 1 else ".mems"
            with open(out + ext, "rb") as f:
                got = f.read()
            assert got == ref[ext] and len(got) > 0, (revcomp, flags)


@need_ref
@pytest.mark.parametrize("producer", ["direct", "pfp", "guided", "packed"])
def test_gpu_stream_through_the_reference_scan(tmp_path, producer):
    """The GPU's own SA / LCP / BWT of small collections, scanned by the reference: equal to the GPU's .mums / .mems."""
    import mumemto_amd
    env_packed = os.environ.get("MMT_PACKED_TEXT")
    if producer == "packed":
        os.environ["MMT_PACKED_TEXT"] = "1"
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_producer("guided" if producer == "packed" else producer, 10, 37)
        eng.keep_columns(True)
        for seed, docs in enumerate([synth.pangenome(6, 20000, 0.01, seed=5, inversion=(2, 3000, 4000)),
                                     random_collection(np.random.default_rng(77)),
                                     synth.pangenome(40, 2000, 0.02, seed=6)]):
            for revcomp in (True, False):
                lens = R.doc_text_lengths(docs, revcomp)
                for p in (dict(max_doc_freq=1), dict(max_doc_freq=0, num_distinct=2)):
                    q = dict(num_distinct=len(docs), max_total_freq=0)
                    q.update(p)
                    eng.set_docs(docs)
                    eng.run(min_match_len=15, use_revcomp=revcomp, **q)
                    sa, lcp, bwt = eng.sa(), eng.lcp(), eng.bwt()
                    assert len(sa) == sum(lens)
                    ref = R.run(sa, lcp, bwt, lens, tmp_path, min_len=15, revcomp=revcomp, **q)
                    assert eng.output_text() == ref[".mums" if p["max_doc_freq"] == 1 else ".mems"], (seed, revcomp, p)
    finally:
        eng.close()
        if producer == "packed":
            if env_packed is None:
                os.environ.pop("MMT_PACKED_TEXT", None)
            else:
                os.environ["MMT_PACKED_TEXT"] = env_packed


@need_ref
def test_large_collection_without_the_c_oracle(tmp_path):
    """94 x 256 kbp (~48 M stream entries): the GPU's stream and .mums against the reference scan alone."""
    import mumemto_amd
    docs = synth.pangenome(94, 256000, 0.001, seed=94)
    eng = mumemto_amd.Engine(0)
    try:
        eng.keep_columns(True)
        eng.set_docs(docs)
        eng.run(min_match_len=20)
        got = eng.output_text()
        lens = R.doc_text_lengths(docs, True)
        ref = R.run(eng.sa(), eng.lcp(), eng.bwt(), lens, tmp_path, min_len=20, timeout=180)
        assert got == ref[".mums"] and got.count(b"\n") > 0
    finally:
        eng.close()


if __name__ == "__main__":                             # test_wide_streams_scan_variants, in a process of its own
    import mumemto_amd
    e = mumemto_amd.Engine(0)
    n = check_wide(e, sys.argv[1], wheres=("both",))
    e.close()
    print("wide ok: %d runs" % n)
