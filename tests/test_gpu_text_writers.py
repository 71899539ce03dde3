"""GPU: the three ways PREFIX.mums / .mems bytes leave the device for a file -- the text sink of a streamed run
(Engine.set_text_sink), the merged table written in pieces (MMT_MERGED_TEXT_PIECE) and the file written at the end of a run
(run_files) -- give the same bytes whatever the piece boundaries are, and a write that fails (a missing directory, a full
device: /dev/full) raises, leaves no PATH.tmp behind and leaves the engine usable."""
import os
import subprocess
import sys

import pytest

if __name__ == "__main__":          # the child of test_sink_ring_wraps_on_a_small_input
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests")]

import mumemto_amd.binding
import pyoracle as O
from mumemto_amd import synth

pytestmark = pytest.mark.gpu
MumemtoError = mumemto_amd.binding.MumemtoError


class env_set:
    """environment variables for the runs inside the block (the library reads them per run)"""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _small_docs():
    return synth.pangenome(7, 40000, 0.01, seed=33, indel_rate=0.0005, inversion=(3, 3000, 9000))


def _parts_of(eng, docs, groups):
    """anchor partitions (documents 0 + a group each) as anchor_merge takes them; the last run holds the anchor's ranks"""
    parts = []
    for g in groups:
        eng.set_docs([docs[i] for i in g])
        eng.run(merge_metadata=True)
        L, off, st = eng.rows_mum()
        parts.append((L, off, st, eng.thresholds()[: len(docs[0][0]) + 1].copy()))
    return parts


def test_pieced_merged_text_equals_one_piece_merged_text(tmp_path):
    import mumemto_amd
    docs = synth.pangenome(7, 20000, 0.01, seed=21, indel_rate=0.001, inversion=(4, 3000, 5000))
    want = O.run(docs, merge=True).text()
    eng = mumemto_amd.Engine(0)
    try:
        parts = _parts_of(eng, docs, [[0, 1, 2], [0, 3, 4], [0, 5, 6]])
        whole, pieced = str(tmp_path / "whole.mums"), str(tmp_path / "pieced.mums")
        eng.anchor_merge(parts, sort_like_direct=True, want_rows=False, text_file=whole)
        with env_set(MMT_MERGED_TEXT_PIECE=4096):
            eng.anchor_merge(parts, sort_like_direct=True, want_rows=False, text_file=pieced)
        got = open(pieced, "rb").read()
        assert len(got) > 3 * 4096, "the table must take several pieces"
        assert got == open(whole, "rb").read() == want
        assert sorted(os.listdir(tmp_path)) == ["pieced.mums", "whole.mums"]
    finally:
        eng.close()


def _ring_child(tmp):
    """MMT_SINK_BLOCK_MB=1 (read when an engine is made: set for this whole process): > 5 MB of PREFIX.mums through a ring of
    four 1 MB blocks, so every block is used again, with windows that put several pieces into a block, about one, and
    pieces larger than a block.  Whether a run ever has to wait for the oldest block is a matter of timing; a block used
    again before it was written would show in the bytes and in the digest."""
    import mumemto_amd
    docs = [[b.tobytes()] for _, b in synth.haplotypes_sparse(32, 1_200_000, 0.001, 9)]
    eng = mumemto_amd.Engine(0)
    eng.set_producer("pfp")
    eng.set_docs(docs)
    eng.run(min_match_len=14)
    want = eng.output_text()
    assert len(want) > 5 << 20, len(want)
    digests = []
    for i, scan_range in enumerate((1 << 20, 1 << 22, 1 << 25)):
        out = os.path.join(tmp, "ring%d.mums" % i)
        with env_set(MMT_SCAN_RANGE=scan_range):
            eng.set_text_sink(out)
            eng.set_docs(docs)
            eng.run(min_match_len=14)
            eng.set_text_sink(None)
        assert eng.stream_stats()["windows"] >= 2
        assert open(out, "rb").read() == want, scan_range
        assert not os.path.exists(out + ".tmp")
        digests.append(eng.text_sink_digest())
        assert eng.output_text() == want                # (a multi-MUM run of this size keeps its rows)
    assert digests[0][0] == len(want) and len(set(digests)) == 1, digests
    eng.close()
    print("ring ok: %d bytes, digest %016x" % digests[0])


def test_sink_ring_wraps_on_a_small_input(tmp_path):
    env = dict(os.environ, MMT_SINK_BLOCK_MB="1", MMT_SINK_DIGEST="1")
    r = subprocess.run([sys.executable, __file__, str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ring ok" in r.stdout


def _full(tmp_path, name):
    """a path whose bytes go to /dev/full (what a caller that appends .mums to a prefix can be given)"""
    os.symlink("/dev/full", str(tmp_path / name))
    return str(tmp_path / name)


def test_a_sink_that_cannot_be_written_fails_the_run_and_nothing_else(tmp_path):
    import mumemto_amd
    docs = _small_docs()
    want = O.run(docs).text()
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_producer("pfp")
        with env_set(MMT_SCAN_RANGE=8192):
            for sink, what in ((str(tmp_path / "nodir" / "out.mums"), "cannot write"), ("/dev/full", "short write to /dev/full")):
                eng.set_text_sink(sink)
                eng.set_docs(docs)
                with pytest.raises(MumemtoError, match=what):
                    eng.run()
                eng.set_text_sink(None)
                assert os.listdir(tmp_path) == []
                # the same engine, a sink that works, and no sink
                out = str(tmp_path / "out.mums")
                eng.set_text_sink(out)
                eng.set_docs(docs)
                eng.run()
                eng.set_text_sink(None)
                assert open(out, "rb").read() == want and os.listdir(tmp_path) == ["out.mums"]
                os.unlink(out)
                eng.set_docs(docs)
                eng.run()
                assert eng.output_text() == want and want.count(b"\n") > 20
    finally:
        eng.set_producer("auto")
        eng.close()


def test_a_merged_text_that_cannot_be_written_fails_and_leaves_nothing(tmp_path):
    import mumemto_amd
    docs = synth.pangenome(7, 20000, 0.01, seed=21, indel_rate=0.001, inversion=(4, 3000, 5000))
    want = O.run(docs, merge=True).text()
    eng = mumemto_amd.Engine(0)
    try:
        parts = _parts_of(eng, docs, [[0, 1, 2], [0, 3, 4], [0, 5, 6]])
        with env_set(MMT_MERGED_TEXT_PIECE=4096):
            for path, what in ((str(tmp_path / "nodir" / "m.mums"), "cannot write"), ("/dev/full", "short write to /dev/full")):
                with pytest.raises(MumemtoError, match=what):
                    eng.anchor_merge(parts, sort_like_direct=True, want_rows=False, text_file=path)
                assert os.listdir(tmp_path) == []
                good = str(tmp_path / "m.mums")
                eng.anchor_merge(parts, sort_like_direct=True, want_rows=False, text_file=good)
                assert open(good, "rb").read() == want and os.listdir(tmp_path) == ["m.mums"]
                os.unlink(good)
    finally:
        eng.close()


def test_a_file_written_at_the_end_of_the_run_that_cannot_be_written(tmp_path):
    import mumemto_amd
    docs = _small_docs()
    want = O.run(docs).text()
    fasta = tmp_path / "in"
    fasta.mkdir()
    paths = []
    for i, d in enumerate(docs):
        paths.append(str(fasta / ("h%d.fa" % i)))
        synth.write_fasta(paths[-1], d)
    out = tmp_path / "out"
    out.mkdir()
    _full(out, "full.mums")
    eng = mumemto_amd.Engine(0)
    try:
        with env_set(MUMEMTO_NO_TEXT_SINK=1):
            for prefix, what in ((str(out / "nodir" / "x"), "cannot write"), (str(out / "full"), "short write to")):
                with pytest.raises(MumemtoError, match=what):
                    eng.run_files(paths, out_prefix=prefix)
                assert sorted(os.listdir(out)) == ["full.mums"]
                eng.run_files(paths, out_prefix=str(out / "good"))
                assert (out / "good.mums").read_bytes() == want and want.count(b"\n") > 20
                assert sorted(os.listdir(out)) == ["full.mums", "good.lengths", "good.mums"]
                os.unlink(str(out / "good.mums"))
                os.unlink(str(out / "good.lengths"))
    finally:
        eng.close()


if __name__ == "__main__":
    _ring_child(sys.argv[1])
