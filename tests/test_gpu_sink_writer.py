"""GPU: the text sink's helper thread prepares the ring and removes an earlier run's file while the sort runs (PieceWriter::Early,
OutFile::retire_old) -- PREFIX.mums that leaves in many pieces is the file the engine returns in memory, over an earlier file or
none; special files are written as before; and a run whose writes fail after the first pieces leaves neither PATH nor PATH.tmp,
whether an earlier PATH was there or not."""
import os
import resource
import signal
import threading

import pytest

import mumemto_amd
import mumemto_amd.binding
from mumemto_amd import synth

pytestmark = pytest.mark.gpu
MumemtoError = mumemto_amd.binding.MumemtoError

# two collections: few long documents, both strands; many short ones (94 columns per row)
COLLECTIONS = {"4x20k": (4, 20000, 0.01, 11), "94x2k": (94, 2000, 0.0005, 12)}


class env_set:
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


@pytest.fixture(scope="module")
def engine():
    eng = mumemto_amd.Engine(0)
    eng.set_producer("pfp")           # (four documents would take the direct sort, which writes its file at the end)
    yield eng
    eng.set_producer("auto")
    eng.close()


@pytest.fixture(scope="module")
def jobs(engine, tmp_path_factory):
    """name -> (FASTA paths, docs, the bytes the engine returns in memory for them)"""
    out = {}
    for name, (haps, length, div, seed) in COLLECTIONS.items():
        docs = synth.pangenome(haps, length, div, seed=seed)
        d = tmp_path_factory.mktemp("fa_" + name)
        paths = []
        for i, doc in enumerate(docs):
            paths.append(str(d / ("h%03d.fa" % i)))
            synth.write_fasta(paths[-1], doc)
        engine.set_docs(docs)
        engine.run()
        want = engine.output_text()
        assert want.count(b"\n") > 15, name
        out[name] = (paths, docs, want)
    return out


@pytest.mark.parametrize("earlier", ["none", "earlier_file"])
@pytest.mark.parametrize("name", sorted(COLLECTIONS))
def test_file_is_what_the_engine_returns_in_memory(engine, jobs, tmp_path, name, earlier):
    paths, _, want = jobs[name]
    prefix = str(tmp_path / "out")
    if earlier == "earlier_file":
        with open(prefix + ".mums", "wb") as f:
            f.write(b"the output of an earlier run\n" * 1000)
    with env_set(MMT_SCAN_RANGE=4096):
        engine.run_files(paths, out_prefix=prefix)
    assert engine.stream_stats()["windows"] > 8           # the output left in many pieces
    got = open(prefix + ".mums", "rb").read()
    assert got == want
    assert os.path.getsize(prefix + ".mums") == engine.text_sink_digest()[0] == len(want)
    assert sorted(os.listdir(tmp_path)) == ["out.lengths", "out.mums"]


@pytest.mark.parametrize("name", sorted(COLLECTIONS))
def test_special_files_are_written_as_before(engine, jobs, tmp_path, name):
    _, docs, want = jobs[name]
    with env_set(MMT_SCAN_RANGE=4096, MMT_SINK_DIGEST=1):
        out = str(tmp_path / "plain.mums")
        engine.set_text_sink(out)
        engine.set_docs(docs)
        engine.run()
        digest_of_the_file = engine.text_sink_digest()
        assert open(out, "rb").read() == want and digest_of_the_file[0] == len(want)
        # /dev/null: the count and the digest of the bytes in file order
        engine.set_text_sink("/dev/null")
        engine.set_docs(docs)
        engine.run()
        assert engine.text_sink_digest() == digest_of_the_file
        # a FIFO read by a thread
        fifo = str(tmp_path / "fifo")
        os.mkfifo(fifo)
        box = []
        reader = threading.Thread(target=lambda: box.append(open(fifo, "rb").read()))
        reader.start()
        try:
            engine.set_text_sink(fifo)
            engine.set_docs(docs)
            engine.run()
        finally:
            engine.set_text_sink(None)
            if reader.is_alive() and not box:
                try:                  # (a run that never opened it must not leave the reader waiting)
                    os.close(os.open(fifo, os.O_WRONLY | os.O_NONBLOCK))
                except OSError:
                    pass
            reader.join()
        assert box[0] == want
        assert engine.text_sink_digest() == digest_of_the_file
    assert sorted(os.listdir(tmp_path)) == ["fifo", "plain.mums"]


def test_a_run_whose_writes_fail_after_the_first_pieces_leaves_nothing(engine, jobs, tmp_path):
    """The file may grow to 4096 bytes (the process's limit for the size of a file, while the run goes on): the first pieces are
    written, a later write is refused.  An earlier PATH is gone when the run starts writing: the failed run leaves no stale one."""
    _, docs, want = jobs["4x20k"]
    assert len(want) > 2 * 4096
    out = str(tmp_path / "out.mums")
    old_handler = signal.signal(signal.SIGXFSZ, signal.SIG_IGN)
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    try:
        with env_set(MMT_SCAN_RANGE=4096):
            for earlier in (False, True):
                if earlier:
                    with open(out, "wb") as f:
                        f.write(b"the output of an earlier run\n")
                engine.set_text_sink(out)
                engine.set_docs(docs)
                resource.setrlimit(resource.RLIMIT_FSIZE, (4096, hard))
                try:
                    with pytest.raises(MumemtoError, match="short write to"):
                        engine.run()
                finally:
                    resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
                assert os.listdir(tmp_path) == []
                # the same engine and sink, unlimited again
                engine.set_docs(docs)
                engine.run()
                assert open(out, "rb").read() == want and os.listdir(tmp_path) == ["out.mums"]
                os.unlink(out)
    finally:
        engine.set_text_sink(None)
        signal.signal(signal.SIGXFSZ, old_handler)
