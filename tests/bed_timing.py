"""GPU box helper: time the BED writer on a seeded table (default 4 M rows x 94 columns, starts ascending in every column,
3000 contigs per sequence, seeded blocks over six rows in ten) stage by stage, all columns in one call, then the text of every
column, against the numpy closed form of tests/bedmodel.py on the same table and box.

  python tests/bed_timing.py [rows] [columns] [contigs per sequence]
"""
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import bedmodel as M
import mumemto_amd

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
ND = int(sys.argv[2]) if len(sys.argv) > 2 else 94
NC = int(sys.argv[3]) if len(sys.argv) > 3 else 3000


def blocks_of(seed=2):
    """bedmodel.make_blocks without its Python loop: runs of 2-8 rows, every tenth run left free"""
    rng = np.random.default_rng(seed)
    size = rng.integers(2, 9, N // 2 + 1)
    first = np.cumsum(size) - size
    keep = (first + size <= N) & (rng.random(len(size)) < 0.9)
    return np.stack([first[keep], first[keep] + size[keep] - 1], axis=1).astype(np.uint32)


t0 = time.perf_counter()
lengths, starts, strands, totals = M.make_rows(1, N, ND)
contigs = M.make_contigs(3, totals, [NC] * ND)
blocks = blocks_of()
print("table: %d rows x %d columns, %.2f GB of starts, %d blocks, %d contigs per sequence, made in %.1f s" %
      (N, ND, starts.nbytes / 1e9, len(blocks), NC, time.perf_counter() - t0), flush=True)
eng = mumemto_amd.Engine(0)
m = mumemto_amd.Merged.from_rows(eng, lengths, starts, strands)
m.set_blocks(blocks)
for rep in range(2):
    t0 = time.perf_counter()
    k = m.bed(contigs, None, 100)
    wall = time.perf_counter() - t0
    s = m.bed_stats()
    print("bed, all columns (run %d): %.1f ms wall, %d records (%d clamped); HIP events: select %.2f, gather %.2f, lookup %.2f ms; "
          "%d batches" % (rep, wall * 1e3, k, s["clamped"], s["select_ms"], s["gather_ms"], s["lookup_ms"], s["batches"]), flush=True)
t0 = time.perf_counter()
texts = [m.bed_text(c) for c in range(ND)]
wall = time.perf_counter() - t0
s = m.bed_stats()
print("text of %d columns: %.1f ms wall (with the copies to the host), HIP events %.2f ms for %.2f GB: %.1f GB/s" %
      (ND, wall * 1e3, s["text_ms"], s["text_bytes"] / 1e9, s["text_bytes"] / 1e6 / max(s["text_ms"], 1e-9)), flush=True)
record_begin, records = m.bed_records()
m.close()
per_col = len(records) // ND
print("bytes: the select reads 8 B and writes 4 B a row; the gather reads 2 x 9 B and writes 17 B, the lookup reads 17 B and "
      "writes 40 B a record and column: %.1f GB for %d records x %d columns" % (83.0 * per_col * ND / 1e9, per_col, ND))
t0 = time.perf_counter()
want = M.bed(lengths, starts, strands, contigs, None, 100, blocks)
t1 = time.perf_counter()
same_text = all(texts[c] == M.text(want[1][int(want[0][c]):int(want[0][c + 1])], contigs[0][c]) for c in (0, ND - 1))
print("numpy closed form on the same table (tests/bedmodel.py): records %.2f s wall, the text of two columns %.2f s; record "
      "offsets equal: %s, records equal: %s, text of the first and last column equal: %s" %
      (t1 - t0, time.perf_counter() - t1, np.array_equal(record_begin, want[0]), np.array_equal(records, want[1]), same_text),
      flush=True)
eng.close()
