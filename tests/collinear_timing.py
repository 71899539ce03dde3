"""GPU box helper: time the collinear blocks of a seeded table (default 4 M rows x 94 columns, a few thousand rearranged
segments) stage by stage, against the reference-equivalent numpy model of tests/collmodel.py on the same table and box.

  python tests/collinear_timing.py [rows] [columns] [segments]
"""
import os
import sys
import tempfile
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import collmodel as M
import mumemto_amd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ND = int(sys.argv[2]) if len(sys.argv) > 2 else 94
SEG = int(sys.argv[3]) if len(sys.argv) > 3 else 3000


def table(seed=1):
    """syntenic chains with SEG disjoint rearranged segments (half inverted in place, half moved behind the end)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 400, N).astype(np.uint32)
    starts = np.empty((N, ND), np.int64)
    strands = np.ones((N, ND), bool)
    wide = rng.random(N) < 0.002                                   # gaps beyond the limit of 1000, in one column each
    wide_col = rng.integers(0, ND, N)
    for j in range(ND):
        gap = rng.integers(0, 120, N)
        gap[wide & (wide_col == j)] += 1500
        starts[:, j] = np.cumsum(gap + np.concatenate(([0], lens[:-1]))) + int(rng.integers(0, 5000))
    end = int(starts.max()) + 1000
    stride = N // max(SEG, 1)
    for k in range(SEG):
        a = k * stride + int(rng.integers(0, stride // 2))
        b = min(a + int(rng.integers(5, min(200, max(6, stride // 2)))), N - 1)
        j = int(rng.integers(0, ND))
        if k & 1:
            starts[a:b + 1, j] += end - int(starts[a, j]) + k * 1_000_000
        else:
            lo, hi = int(starts[a, j]), int(starts[b, j] + lens[b])
            starts[a:b + 1, j] = lo + hi - (starts[a:b + 1, j] + lens[a:b + 1])
            strands[a:b + 1, j] = False
    return lens, starts, strands


t0 = time.perf_counter()
lens, starts, strands = table()
print("table: %d rows x %d columns, %d segments, %.2f GB of starts, made in %.1f s" % (N, ND, SEG, starts.nbytes / 1e9,
                                                                                     time.perf_counter() - t0), flush=True)
eng = mumemto_amd.Engine(0)
t0 = time.perf_counter()
m = mumemto_amd.Merged.from_rows(eng, lens, starts, strands)
print("upload: %.2f s" % (time.perf_counter() - t0), flush=True)
for rep in range(2):
    t0 = time.perf_counter()
    blk = m.collinear(1000)
    wall = time.perf_counter() - t0
    s = m.collinear_stats()
    print("collinear (run %d): %.1f ms wall, %d blocks; HIP events: filter+sort %.1f, extraction %.1f, sorts %.1f (%d columns; %d "
          "ascending), adjacency %.1f, blocks %.1f ms; %d batch(es)" % (rep, wall * 1e3, len(blk), s["filter_sort_ms"], s["extract_ms"],
                                                                       s["sort_ms"], s["cols_sorted"], s["cols_ascending"],
                                                                       s["adjacency_ms"], s["blocks_ms"], s["batches"]), flush=True)
tb = 8.0 * N * ND
print("bytes against the table's 8 B x rows x columns = %.2f GB:" % (tb / 1e9))
print("  extraction  reads 9 B and writes 8 B a cell: %.2f x the table, %.0f GB/s" % (17 / 8, 17.0 * N * ND / s["extract_ms"] / 1e6))
print("  sorts       %d columns x 12 B a pair and pass, in and out" % s["cols_sorted"])
print("  adjacency   8 B a key (+ 4 B a row number in sorted columns) read, <= 4 + 12 + 12 B a pair read and written: "
      "<= %.2f x the table, %.0f GB/s at that bound" % (40 / 8, 40.0 * N * ND / max(s["adjacency_ms"], 1e-3) / 1e6))
with tempfile.TemporaryDirectory() as d:
    t0 = time.perf_counter()
    m.write_text(os.path.join(d, "sorted.mums"))
    wall = time.perf_counter() - t0
    size = os.path.getsize(os.path.join(d, "sorted.mums"))
print("formatting + copy + file: %.2f s wall for %.2f GB of text" % (wall, size / 1e9), flush=True)
t0 = time.perf_counter()
rows = M.prepare(lens, starts, strands)
want = M.blocks(*rows, max_break=1000)
print("numpy model (tests/collmodel.py) on the same table: %.1f s wall; blocks equal: %s" % (time.perf_counter() - t0,
                                                                                         bool(np.array_equal(want, blk))))
m.close()
eng.close()
