"""GPU box helper: time the coverage on a seeded table (default 4 M rows x 94 columns of tests/covmodel.make_table: random
overlapping intervals, a tenth of the cells absent, rows in random order, so every column is sorted) stage by stage, all
columns in one call, against the numpy closed form of tests/covmodel.py on the same table and box.  A second pass orders the
rows by the first column, which then takes the route without a sort.

  python tests/coverage_timing.py [rows] [columns]
"""
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import covmodel as M
import mumemto_amd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ND = int(sys.argv[2]) if len(sys.argv) > 2 else 94


def table(seed=1):
    """covmodel.make_table without its Python loops over rows: lengths, uniform starts, a tenth of the cells absent"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 400, N).astype(np.uint32)
    lengths[rng.random(N) < 0.05] *= 8
    seq_lengths = ((rng.integers(90, 110, ND) * int(lengths.sum() / 0.6)) // 100).astype(np.int64)
    starts = np.empty((N, ND), np.int64)
    for c in range(ND):
        starts[:, c] = rng.integers(0, seq_lengths[c] + 50, N)
        starts[rng.random(N) < 0.1, c] = -1
    return lengths, starts, np.ones((N, ND), bool), seq_lengths


t0 = time.perf_counter()
lengths, starts, strands, seq_lengths = table()
print("table: %d rows x %d columns, %.2f GB of starts, made in %.1f s" % (N, ND, starts.nbytes / 1e9, time.perf_counter() - t0),
      flush=True)
eng = mumemto_amd.Engine(0)
for order in ("random", "by column 0"):
    if order != "random":
        perm = np.argsort(starts[:, 0], kind="stable")
        lengths, starts = lengths[perm], starts[perm]
    m = mumemto_amd.Merged.from_rows(eng, lengths, starts, strands)
    for rep in range(2):
        t0 = time.perf_counter()
        covered = m.coverage(seq_lengths)
        wall = time.perf_counter() - t0
        s = m.coverage_stats()
        print("coverage, rows in %s order (run %d): %.1f ms wall, %d runs; HIP events: extraction %.2f, sorts %.2f (%d columns; %d "
              "ascending), running maximum + sum %.2f, runs %.2f ms; %d batches" %
              (order, rep, wall * 1e3, s["runs"], s["extract_ms"], s["sort_ms"], s["cols_sorted"], s["cols_ascending"], s["scan_ms"],
               s["runs_ms"], s["batches"]), flush=True)
    run_begin, runs = m.coverage_runs()
    m.close()
cells = N * ND
print("bytes: extraction reads 8 B a cell and writes 16 B: %.1f GB; a sorted column moves 16 B a cell and pass, in and out; the "
      "running maximum reads 24 B and writes 12 B a cell: %.1f GB; the runs read 32 B a cell: %.1f GB" %
      (24.0 * cells / 1e9, 36.0 * cells / 1e9, 32.0 * cells / 1e9))
t0 = time.perf_counter()
want = M.coverage(lengths, starts, seq_lengths)
print("numpy closed form on the same table (tests/covmodel.py): %.2f s wall; covered equal: %s, runs equal: %s" %
      (time.perf_counter() - t0, np.array_equal(covered, want[0]), np.array_equal(run_begin, want[1]) and np.array_equal(runs, want[2])),
      flush=True)
eng.close()
