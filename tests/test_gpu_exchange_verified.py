"""GPU: the exchange of dist.cpp verifies every message with digests -- shown over a transport that damages one
received piece (tests/corrupt_rccl, in front of the transport double of tests/fake_rccl).

The collection and the worker pattern are those of test_gpu_exchange_ranks.py (9 haplotypes x 30,000, seed 71; ranks = processes
sharing GPU 0, at most four).  A clean run must still give the oracle's bytes, with every rank's verify_stats() showing digested
pieces and no mismatch; a run with one damaged piece must END ON EVERY RANK (a verdict only the detecting rank knew would leave
the others waiting in the next collective), non-zero, inside the time limit, with no merged.mums, the detecting rank naming peer,
table and bytes and every other rank naming the detecting rank.

Which receive a plan `rank:dtype:ordinal:mode` hits follows from the order dist.cpp posts its receives in: peers in rank order
and, within a peer, lengths (u32), offsets (i64), strands (u8), thresholds (u32), each in pieces of MUMEMTO_RCCL_CHUNK elements
(one piece by default); the trailer of digests (u64) behind them.  recv_order() restates that, with the table sizes taken from
the oracle's run of each rank's partition.  Only the sharded gather has no u32 / i64 receives: its one case is the u8 text."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest

import pyoracle as O
from mumemto_amd import synth
from mumemto_amd import dist as mdist
from test_gpu_exchange_ranks import fake_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_DIR = os.path.join(ROOT, "tests", "corrupt_rccl")
SHIM = os.path.join(SHIM_DIR, "libcorrupt_rccl.so")
HAPS, LENGTH, SEED = 9, 30000, 71
RUN_TIMEOUT = 120                      # a hang is a failure, not a stall


def shim_lib():
    if not os.path.exists(SHIM) or os.path.getmtime(SHIM) < os.path.getmtime(os.path.join(SHIM_DIR, "corrupt_rccl.cpp")):
        subprocess.check_call(["make", "-C", SHIM_DIR])
    return SHIM


_WORKER = r"""
import json, os, sys, time, traceback
root = %(root)r
sys.path[:0] = [root, os.path.join(root, "oracle"), os.path.join(root, "tests")]
import mumemto_amd
from mumemto_amd import synth
from mumemto_amd import dist as mdist
rank, world, idfile, outdir, what = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
docs = synth.pangenome(%(haps)d, %(length)d, 0.01, seed=%(seed)d, inversion=(2, 2000, 5000), indel_rate=0.0005)
eng = mumemto_amd.Engine(0)
if rank == 0:
    uid = mumemto_amd.Comm.unique_id()
    with open(idfile + ".tmp", "wb") as f: f.write(uid)
    os.rename(idfile + ".tmp", idfile)
else:
    t0 = time.time()
    while not os.path.exists(idfile):
        assert time.time() - t0 < 100
        time.sleep(0.01)
    uid = open(idfile, "rb").read()
comm = mumemto_amd.Comm(eng, rank, world, uid)
code = 0
try:
    if what in ("rank0", "ranges"):
        eng.run_partitioned([docs[i] for i in mdist.partition_docs(len(docs), world)[rank]], merge_metadata=True)
        m = comm.merge(by_ranges=(what == "ranges"))
        assert (m is not None) == (rank == 0)
        if rank == 0:
            open(os.path.join(outdir, "merged.mums"), "wb").write(m["text"])
    else:
        eng.set_docs(docs)
        eng.set_scan_shard(rank, world)
        eng.run(num_distinct=%(haps)d - 1, max_doc_freq=3, max_total_freq=3 * %(haps)d)
        text = comm.gather_text()
        if rank == 0:
            open(os.path.join(outdir, "merged.mums"), "wb").write(text)
    print("RANK_OK", rank, flush=True)
except BaseException:
    sys.stderr.write("rank %%d:\n%%s" %% (rank, traceback.format_exc()))
    code = 1
with open(os.path.join(outdir, "stats_%%d.json" %% rank), "w") as f:
    json.dump(comm.verify_stats(), f)
comm.close(); eng.close()
sys.stdout.flush(); sys.stderr.flush()
os._exit(code)
"""


def run_ranks(world, what, plan=None, env_extra=None, env_of_rank=None):
    """One worker process per rank (world <= 4) over the shim.  Returns (return codes, stderrs, stats, merged bytes or None)."""
    assert world <= 4
    with tempfile.TemporaryDirectory(prefix="verified_", dir="/dev/shm") as d:
        script = os.path.join(d, "worker.py")
        with open(script, "w") as f:
            f.write(_WORKER % dict(root=ROOT, haps=HAPS, length=LENGTH, seed=SEED))
        procs = []
        for r in range(world):
            env = dict(os.environ, MUMEMTO_RCCL_LIB=shim_lib(), CORRUPT_RCCL_INNER=fake_lib(), MUMEMTO_NO_TORCH="1",
                       FAKE_RCCL_TIMEOUT="20")
            env.pop("CORRUPT_RCCL_PLAN", None)
            if plan:
                env["CORRUPT_RCCL_PLAN"] = plan
            env.update(env_extra or {})
            env.update((env_of_rank or {}).get(r, {}))
            procs.append(subprocess.Popen([sys.executable, script, str(r), str(world), os.path.join(d, "id"), d, what], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=RUN_TIMEOUT))
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
        stats = []
        for r in range(world):
            path = os.path.join(d, "stats_%d.json" % r)
            stats.append(json.load(open(path)) if os.path.exists(path) else None)
        merged = os.path.join(d, "merged.mums")
        data = open(merged, "rb").read() if os.path.exists(merged) else None
        return [p.returncode for p in procs], [o[1] for o in outs], stats, data


@functools.lru_cache(maxsize=None)
def collection():
    return synth.pangenome(HAPS, LENGTH, 0.01, seed=SEED, inversion=(2, 2000, 5000), indel_rate=0.0005)


@functools.lru_cache(maxsize=None)
def direct_bytes(world):
    docs = collection()
    order = mdist.merged_column_order(mdist.partition_docs(HAPS, world))
    return O.run([docs[i] for i in order], merge=True).text()


@functools.lru_cache(maxsize=None)
def sharded_bytes():
    return O.run(collection(), num_distinct=HAPS - 1, max_doc_freq=3, max_total_freq=3 * HAPS).text()


@functools.lru_cache(maxsize=None)
def partition_tables(world, rank):
    """(rows, cells, thresholds) of the partition rank `rank` sends in route rank0: the oracle's run of its documents."""
    docs = collection()
    lengths, offsets, _ = O.run([docs[i] for i in mdist.partition_docs(HAPS, world)[rank]], merge=True).mum_rows()
    return len(lengths), int(offsets.size), len(docs[0][0]) + 1


def recv_order_rank0(world, chunk=None):
    """The receives of rank 0 in route rank0, one entry per piece: (dtype, table, peer, piece, bytes)."""
    out = []
    for peer in range(1, world):
        rows, cells, L = partition_tables(world, peer)
        for dtype, width, table, n in (("u32", 4, "lengths", rows), ("i64", 8, "offsets", cells), ("u8", 1, "strands", cells),
                                       ("u32", 4, "thresholds", L)):
            if table != "thresholds" and not rows:
                continue
            c = chunk or (1 << 29) // width
            for piece in range(max(1, -(-n // c))):
                out.append((dtype, table, peer, piece, min(c, n - piece * c) * width))
    return out


def pick(order, dtype, which):
    """Ordinal of a receive among those of its datatype with at least two elements (what the shim counts)."""
    width = {"u8": 1, "u32": 4, "i64": 8}[dtype]
    mine = [e for e in order if e[0] == dtype and e[4] >= 2 * width]
    ordinal = which if which >= 0 else len(mine) + which
    return ordinal, mine[ordinal]


def assert_clean(codes, errs, stats):
    assert codes == [0] * len(codes), "\n".join(e[-3000:] for e in errs)
    for r, s in enumerate(stats):
        assert s["pieces"] > 0 and s["bytes"] > 0 and s["messages"] > 0, (r, s)
        assert s["mismatches"] == 0 and s["first_mismatch"] is None, (r, s)


def assert_detected(codes, errs, stats, data, detecting, peer, table, piece=None, nbytes=None):
    assert all(c not in (0, None) for c in codes), (codes, [e[-1500:] for e in errs])
    assert data is None, "merged.mums was written although a piece arrived damaged"
    for r, e in enumerate(errs):
        assert "exchange verification failed" in e and "rank %d detected" % detecting in e, (r, e[-3000:])
    e = errs[detecting]
    assert "from peer %d, table %s, " % (peer, table) in e, e[-3000:]
    assert " bytes" in e.split("table %s, " % table)[1][:60], e[-3000:]
    if piece is not None:
        assert "table %s, piece %d, " % (table, piece) in e, e[-3000:]
    if nbytes is not None:
        assert "piece %d, %d bytes" % (piece, nbytes) in e, e[-3000:]
    first = stats[detecting]["first_mismatch"]
    assert stats[detecting]["mismatches"] >= 1 and first["peer"] == peer and first["table"] == table, stats[detecting]
    for r, s in enumerate(stats):
        if r != detecting:
            assert s["mismatches"] == 0, (r, s)


# ---- clean runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,what", [(2, "rank0"), (3, "rank0"), (3, "ranges"), (4, "ranges"), (2, "sharded")])
def test_clean_runs_verify_and_give_the_oracles_bytes(world, what):
    codes, errs, stats, data = run_ranks(world, what)
    assert_clean(codes, errs, stats)
    want = sharded_bytes() if what == "sharded" else direct_bytes(world)
    assert want.count(b"\n") > 10 and data == want


def test_clean_run_in_dozens_of_pieces():
    codes, errs, stats, data = run_ranks(3, "ranges", env_extra={"MUMEMTO_RCCL_CHUNK": "997"})
    assert_clean(codes, errs, stats)
    assert data == direct_bytes(3)
    assert all(s["pieces"] >= 24 for s in stats), stats        # (a third of the 30,001 thresholds alone is 11 pieces a message)


# ---- one damaged piece -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,which,table", [("u32", 0, "lengths"), ("u32", -1, "thresholds"), ("i64", 0, "offsets"),
                                               ("u8", 0, "strands")])
def test_flip_on_rank_0_of_the_rank0_route(dtype, which, table):
    ordinal, (_, want_table, peer, piece, nbytes) = pick(recv_order_rank0(2), dtype, which)
    assert want_table == table and peer == 1
    codes, errs, stats, data = run_ranks(2, "rank0", plan="0:%s:%d:flip" % (dtype, ordinal))
    assert_detected(codes, errs, stats, data, 0, 1, table, piece, nbytes)


# route ranges, world 3, rank 1 in the slice step: it receives from rank 0 then rank 2, from each lengths (u32), offsets (i64),
# strands (u8) of the rows that start in its third of the anchor (each partition has ~500 rows: far more than two) and thresholds
# (u32) -- u32 ordinals 0 .. 3 = lengths 0, thresholds 0, lengths 2, thresholds 2.  Rank 1 receives nothing in the second step.
@pytest.mark.parametrize("dtype,ordinal,table,peer", [("u32", 0, "lengths", 0), ("u32", 3, "thresholds", 2), ("i64", 0, "offsets", 0),
                                                      ("u8", 0, "strands", 0)])
def test_flip_on_rank_1_of_the_slice_step_ends_every_rank(dtype, ordinal, table, peer):
    codes, errs, stats, data = run_ranks(3, "ranges", plan="1:%s:%d:flip" % (dtype, ordinal))
    assert_detected(codes, errs, stats, data, 1, peer, table, 0)
    assert stats[1]["messages"] == 16        # 8 sent + 8 received in the slice step, and nothing after it


def test_flip_in_the_second_step_of_the_range_route():
    """Rank 0 of a world of 3 receives two i64 messages in the slice step (offsets from ranks 1 and 2): i64 ordinal 2 is the
    offsets of rank 1's folded piece, which arrives after the fold."""
    codes, errs, stats, data = run_ranks(3, "ranges", plan="0:i64:2:flip")
    assert_detected(codes, errs, stats, data, 0, 1, "offsets", 0)
    assert stats[0]["messages"] == 16 + 8   # the slice step verified clean (8 sent + 8 received), then the 8 of the pieces


def test_flip_in_the_gathered_text_of_the_sharded_route():
    codes, errs, stats, data = run_ranks(2, "sharded", plan="0:u8:0:flip")
    assert_detected(codes, errs, stats, data, 0, 1, "text", 0)


@pytest.mark.parametrize("mode,which", [("swap", 1), ("zero_tail", -1)])
def test_the_damaged_piece_is_named(mode, which):
    """MUMEMTO_RCCL_CHUNK=997: the offsets of rank 1 (2,760 cells) travel as three pieces; the i64 ordinal that is damaged is
    the piece that is named.  Offsets are distinct, so the halves of a piece differ."""
    order = recv_order_rank0(2, chunk=997)
    ordinal, (_, table, peer, piece, nbytes) = pick(order, "i64", which)
    assert table == "offsets" and piece == ordinal and len([e for e in order if e[0] == "i64"]) >= 3
    codes, errs, stats, data = run_ranks(2, "rank0", plan="0:i64:%d:%s" % (ordinal, mode), env_extra={"MUMEMTO_RCCL_CHUNK": "997"})
    assert_detected(codes, errs, stats, data, 0, 1, "offsets", piece, nbytes)
    assert stats[0]["first_mismatch"]["piece"] == ordinal and stats[0]["mismatches"] == 1


def test_a_damaged_trailer_is_told_from_damaged_data():
    codes, errs, stats, data = run_ranks(2, "rank0", plan="0:u64:0:flip")
    assert_detected(codes, errs, stats, data, 0, 1, "digests", 0)


# ---- the switch ------------------------------------------------------------------------------------------------------------
def test_verification_off_lets_the_damage_through():
    """MUMEMTO_EXCHANGE_VERIFY=0: no digests, no trailers -- the same damaged threshold (its low bit: harmless to the fold's
    indexing) goes unnoticed, so the failures above come from the verification.  (The bytes are not compared.)"""
    ordinal, (_, table, _, _, _) = pick(recv_order_rank0(2), "u32", -1)
    assert table == "thresholds"
    codes, errs, stats, data = run_ranks(2, "rank0", plan="0:u32:%d:flip" % ordinal, env_extra={"MUMEMTO_EXCHANGE_VERIFY": "0"})
    assert codes == [0, 0], "\n".join(e[-3000:] for e in errs)
    assert data is not None and all(s["pieces"] == 0 and s["bytes"] == 0 for s in stats), stats


def test_rank_0_decides_about_the_switch():
    codes, errs, stats, data = run_ranks(2, "rank0", env_of_rank={1: {"MUMEMTO_EXCHANGE_VERIFY": "0"}})
    assert_clean(codes, errs, stats)
    assert data == direct_bytes(2)


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_mumemto_exec_gpus_2_fails_on_a_damaged_piece_and_leaves_no_output(tmp_path):
    exe = os.path.join(ROOT, "mumemto_amd", "bin", "mumemto_exec")
    docs = synth.pangenome(9, 30000, 0.01, seed=79, inversion=(3, 2000, 5000))
    paths = []
    for i, d in enumerate(docs):
        p = str(tmp_path / ("h%02d.fa" % i))
        synth.write_fasta(p, d)
        paths.append(p)
    env = dict(os.environ, MUMEMTO_RCCL_LIB=shim_lib(), CORRUPT_RCCL_INNER=fake_lib(), MUMEMTO_SHARE_DEVICE="1", FAKE_RCCL_TIMEOUT="20")
    env.pop("CORRUPT_RCCL_PLAN", None)
    order = mdist.merged_column_order(mdist.partition_docs(9, 2))
    want = O.run([docs[i] for i in order], merge=True).text()
    clean = str(tmp_path / "clean")
    r = subprocess.run([exe, "-o", clean, "--gpus", "2", "-n"] + paths, capture_output=True, text=True, timeout=RUN_TIMEOUT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert open(clean + ".mums", "rb").read() == want
    # rank 0 receives lengths (u32, hundreds of rows), offsets, strands, thresholds (u32) from rank 1: u32 ordinal 1
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "-o", out, "--gpus", "2", "-n"] + paths, capture_output=True, text=True, timeout=RUN_TIMEOUT,
                       env=dict(env, CORRUPT_RCCL_PLAN="0:u32:1:flip"))
    assert r.returncode != 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "exchange verification failed" in r.stderr and "rank 0 detected" in r.stderr, r.stderr[-4000:]
    assert "from peer 1, table thresholds, piece 0, %d bytes" % (4 * (len(docs[0][0]) + 1)) in r.stderr, r.stderr[-4000:]
    assert not os.path.exists(out + ".mums")
