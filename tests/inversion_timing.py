"""GPU box helper: time the inversion caller on a seeded table (default 4 M rows x 94 columns, 5 % of the rows in inverted
segments that gaps above the limit break into several blocks) stage by stage, against the reference-equivalent numpy model
of tests/invmodel.py on the same table and box.

  python tests/inversion_timing.py [rows] [columns] [inverted fraction]
"""
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import collmodel
import invmodel as M
import mumemto_amd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ND = int(sys.argv[2]) if len(sys.argv) > 2 else 94
FRAC = float(sys.argv[3]) if len(sys.argv) > 3 else 0.05
SEG_ROWS = 400


def table(seed=1):
    """syntenic chains; a gap beyond the limit of 1000 in one column in front of 1 % of the rows; disjoint segments of
    SEG_ROWS rows, FRAC of all rows, each inverted in place in one column"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 400, N).astype(np.uint32)
    starts = np.empty((N, ND), np.int64)
    strands = np.ones((N, ND), bool)
    wide = rng.random(N) < 0.01
    wide_col = rng.integers(0, ND, N)
    for j in range(ND):
        gap = rng.integers(0, 120, N)
        gap[wide & (wide_col == j)] += 1500
        starts[:, j] = np.cumsum(gap + np.concatenate(([0], lens[:-1]))) + int(rng.integers(0, 5000))
    segments = max(int(N * FRAC / SEG_ROWS), 1)
    stride = N // segments
    for k in range(segments):
        a = k * stride + int(rng.integers(0, max(stride - SEG_ROWS, 1)))
        b = min(a + SEG_ROWS - 1, N - 1)
        j = 1 + int(rng.integers(0, ND - 1))
        lo, hi = int(starts[a, j]), int(starts[b, j] + lens[b])
        starts[a:b + 1, j] = lo + hi - (starts[a:b + 1, j] + lens[a:b + 1])
        strands[a:b + 1, j] = False
    return lens, starts, strands, segments


t0 = time.perf_counter()
lens, starts, strands, segments = table()
print("table: %d rows x %d columns, %d inverted segments, %.2f GB of starts, made in %.1f s" %
      (N, ND, segments, starts.nbytes / 1e9, time.perf_counter() - t0), flush=True)
eng = mumemto_amd.Engine(0)
m = mumemto_amd.Merged.from_rows(eng, lens, starts, strands)
t0 = time.perf_counter()
blk = m.collinear(1000)
print("collinear: %.1f ms wall, %d blocks" % ((time.perf_counter() - t0) * 1e3, len(blk)), flush=True)
for rep in range(2):
    t0 = time.perf_counter()
    calls = m.inversions()
    wall = time.perf_counter() - t0
    s = m.inversion_stats()
    print("inversions (run %d): %.1f ms wall, %d calls of %d runs; HIP events: gather %.2f, sorts %.2f (%d columns; %d ascending), "
          "run passes %.2f ms" % (rep, wall * 1e3, len(calls), s["runs"], s["gather_ms"], s["sort_ms"], s["cols_sorted"],
                                  s["cols_ascending"], s["runs_ms"]), flush=True)
print("bytes: gather reads 9 B a block head and column and writes 8 B: %.1f MB; a sorted column moves 12 B a block and pass, in and "
      "out; the run passes read and write ~30 B a block" % (17.0 * len(blk) * (ND - 1) / 1e6))
t0 = time.perf_counter()
rows = collmodel.prepare(lens, starts, strands)
t1 = time.perf_counter()
want_blk = collmodel.blocks(*rows, max_break=1000)
t2 = time.perf_counter()
want = M.calls(*rows, want_blk)
t3 = time.perf_counter()
print("numpy model on the same table: prepare %.1f s, blocks %.1f s, calls (tests/invmodel.py) %.2f s wall; calls equal: %s" %
      (t1 - t0, t2 - t1, t3 - t2, np.array_equal(calls, want)), flush=True)
m.close()
eng.close()
