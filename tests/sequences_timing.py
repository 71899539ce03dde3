"""GPU box helper: time the multi-MUM sequence writer (csrc/sequences.cpp, sequence_kernels.hip) on one MI355X, in output bytes
per second of the format pass (HIP events) and of the whole call (host clock: measure, format, copy out, file written), on

  run    the MUM rows of a run of bench.py's collection (synth.collection_sparse; --haps / --length scale it), column 0,
         read from the engine's resident text
  long   a synthetic table of long records only (--records x --record-length bases of document 0), both strands

against two baselines measured in the same session: a device-to-device copy of as many bytes as the text has (the ceiling:
the kernel reads and writes every byte once), and the host-only extract_mums binary on the same table and FASTA file (wall
time of its second run: the page cache is warm).  Warm-up first, then the median of --repeats.

  python tests/sequences_timing.py [--haps N] [--length L] [--records R] [--record-length B] [--repeats K]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import torch
from mumemto_amd import binding, build, mumsio, synth

ap = argparse.ArgumentParser()
ap.add_argument("--haps", type=int, default=94)
ap.add_argument("--length", type=int, default=64_000_000)
ap.add_argument("--divergence", type=float, default=0.001)
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--records", type=int, default=2000)
ap.add_argument("--record-length", type=int, default=200_000)
ap.add_argument("--repeats", type=int, default=7)
A = ap.parse_args()
import mumemto_amd  # noqa: E402

BINARY = os.path.join(build.BIN_DIR, "extract_mums")


def copy_rate(n_bytes):
    """GB/s of a device-to-device copy of n_bytes (hipMemcpy through torch), median of the repeats"""
    src = torch.full((n_bytes,), 65, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    times = []
    for rep in range(A.repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return n_bytes / statistics.median(times[2:]) / 1e6


def device(m, col, source, dialect, path):
    """-> (text bytes, format ms median, whole-call s median, measure ms)"""
    fmt, whole, measure = [], [], 0.0
    for rep in range(A.repeats + 2):
        t0 = time.perf_counter()
        n_bytes = m.sequences(col, source, dialect)
        m.write_sequences(path)
        whole.append(time.perf_counter() - t0)
        s = m.sequences_stats()
        fmt.append(s["format_ms"])
        measure = s["measure_ms"]
    return n_bytes, statistics.median(fmt[2:]), statistics.median(whole[2:]), measure


def host_binary(work, name, table, fasta, n_seqs):
    """wall seconds of the second run of the extract_mums binary, and its output"""
    mumsio.write_mums(os.path.join(work, name + ".mums"), *table)
    with open(os.path.join(work, name + ".lengths"), "w") as f:
        f.write("".join("%s 0\n" % fasta for _ in range(n_seqs)))
    out = os.path.join(work, name + "_mums.fa")
    for rep in range(2):
        t0 = time.perf_counter()
        subprocess.check_call([BINARY, "-m", os.path.join(work, name + ".mums")])
        wall = time.perf_counter() - t0
    return wall, out


def same_file(a, b):
    return subprocess.run(["cmp", "-s", a, b]).returncode == 0


def report(name, n_bytes, fmt_ms, whole_s, measure_ms, copy, host_s, equal):
    print("%-5s %8.1f MB of text: format pass %8.3f ms = %7.1f GB/s (%.0f%% of the %.0f GB/s copy), measure %.3f ms; whole call "
          "%.3f s = %.2f GB/s; extract_mums binary %.3f s = %.2f GB/s (whole call %.1fx); same bytes: %s" %
          (name, n_bytes / 1e6, fmt_ms, n_bytes / fmt_ms / 1e6, 100 * n_bytes / fmt_ms / 1e6 / copy, copy, measure_ms, whole_s,
           n_bytes / whole_s / 1e9, host_s, n_bytes / host_s / 1e9, host_s / whole_s, equal), flush=True)


t0 = time.perf_counter()
bases, lens = synth.collection_sparse(A.haps, A.length, A.divergence, A.seed)
eng = mumemto_amd.Engine(0)
eng.set_docs([[bases[int(sum(lens[:d])):int(sum(lens[:d + 1]))].tobytes()] for d in range(len(lens))])
eng.run()
rows = eng.rows_mum()
print("%d haplotypes x %d bp: %d MUM rows, %d bases in column 0, text %s, made and run in %.1f s" %
      (A.haps, A.length, len(rows[0]), int(rows[0].sum()), "packed" if eng.text_packed() else "bytes", time.perf_counter() - t0), flush=True)
doc0 = bases[:int(lens[0])].tobytes()
with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as work:
    fasta = os.path.join(work, "doc0.fa")
    synth.write_fasta_fast(fasta, bases[:int(lens[0])])
    ours = os.path.join(work, "ours.fa")
    # ---- the rows of the run, from the resident text ----------------------------------------------------------------------
    with mumemto_amd.Merged.from_device(eng, *eng.rows_mum_device()) as m:
        n_bytes, fmt_ms, whole_s, measure_ms = device(m, 0, None, "binary", ours)
    host_s, theirs = host_binary(work, "run", (rows[0], rows[1], rows[2].astype(bool)), fasta, len(lens))
    report("run", n_bytes, fmt_ms, whole_s, measure_ms, copy_rate(n_bytes), host_s, same_file(ours, theirs))
    # ---- long records only ----------------------------------------------------------------------------------------------
    rng = np.random.default_rng(A.seed)
    n = A.records
    length = min(A.record_length, len(doc0) // 2)
    table = (np.full(n, length, np.uint32), rng.integers(0, len(doc0) - length, size=(n, 1)), np.ones((n, 1), bool))
    host_s, theirs = host_binary(work, "long", table, fasta, 1)
    for name, dialect, strands in (("long+", "binary", table[2]), ("long-", "python", ~table[2])):
        with mumemto_amd.Merged.from_rows(eng, table[0], table[1], strands) as m:
            n_bytes, fmt_ms, whole_s, measure_ms = device(m, 0, doc0, dialect, ours)
        report(name, n_bytes, fmt_ms, whole_s, measure_ms, copy_rate(n_bytes), host_s, same_file(ours, theirs) if dialect == "binary" else "-")
eng.close()
