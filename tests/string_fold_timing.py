"""GPU box helper: time the string fold (mumemto_amd/csrc/string_fold.cpp) stage by stage on a seeded workload -- by default 4
partitions of 2 columns, 4 M rows of mom that each cover one record of every collection (so nearly 4 M merged rows) and row
lengths of 20 .. 980, about 2 G positions -- and the numpy closed form (merge_mums.string_merge) on the same box at a quarter
of that size, in a process of its own for its peak RSS.  That process is started first, while this one holds nothing: a child's
ru_maxrss begins at its parent's high-water mark, so a model started beside the 32 GB workload would report the workload.
Every partition has the same row lengths and row g of mom is record g everywhere, so all 2 S tables are read front to back
at the same pace: the layout a streaming pass likes best.

  python tests/string_fold_timing.py [rows] [partitions] [model rows]
  python tests/string_fold_timing.py model ROWS PARTITIONS          (the closed form alone, no GPU needed)

HIP-event times per stage come from mmt_merged_string_fold_stats; the threshold pass is rated against its algorithmic traffic,
(4 S + 4) bytes per output position: S values of either table read, two written."""
import os
import resource
import subprocess
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np

argv = sys.argv[1:]
ONLY_MODEL = bool(argv) and argv[0] == "model"
argv = argv[1:] if ONLY_MODEL else argv
N = int(argv[0]) if len(argv) > 0 else 4_000_000
S = int(argv[1]) if len(argv) > 1 else 4
N_MODEL = int(argv[2]) if len(argv) > 2 else max(N // 4, 1)
COLS = 2


def workload(n, s, seed=11):
    """-> parts, mom, records: every partition has the same row lengths (so row g of mom is record g everywhere), its own starts
    and threshold tables of 1 .. 15 repeated from a block of 2^20 values; mom matches reversed in a third of the other collections"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(20, 981, n).astype(np.uint32)
    total = int((lengths.astype(np.int64) + 1).sum())
    records = lengths.astype(np.int64) + 1
    records[-1] = max(1, records[-1] // 2)
    begin = np.cumsum(records) - records
    parts = []
    for i in range(s):
        starts = rng.integers(0, 1 << 38, (n, COLS)).astype(np.int64)
        starts[:, 0] = np.cumsum(lengths.astype(np.int64) + rng.integers(0, 40, n))
        strands = rng.random((n, COLS)) < 0.7
        tables = [np.resize(rng.integers(1, 16, 1 << 20).astype(np.uint16), total) for _ in range(2)]
        parts.append((lengths, starts, strands, tables[0], tables[1]))
    mom_strands = rng.random((n, s)) < 0.67
    mom_strands[:, 0] = True
    mom = (lengths.copy(), np.repeat(begin[:, None], s, axis=1), mom_strands)
    return parts, mom, [records] * s


if ONLY_MODEL:
    from mumemto_amd import merge_mums
    parts, mom, records = workload(N, S)
    t0 = time.perf_counter()
    out = merge_mums.string_merge(parts, mom, records)
    wall = time.perf_counter() - t0
    print("numpy closed form: %d rows of mom, %d partitions -> %d rows, %d positions: %.2f s wall, peak RSS %.2f GB (inputs included)" %
          (N, S, len(out[0]), len(out[3]), wall, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6), flush=True)
    sys.exit(0)

r = subprocess.run([sys.executable, os.path.abspath(__file__), "model", str(N_MODEL), str(S)], capture_output=True, text=True)
print(r.stdout.strip() or r.stderr.strip()[-2000:], flush=True)

import mumemto_amd
from mumemto_amd import merge_mums

t0 = time.perf_counter()
parts, mom, records = workload(N, S)
in_bytes = sum(a.nbytes for p in parts for a in p) + sum(a.nbytes for a in mom)
print("workload: %d rows of mom, %d partitions x %d columns, %.2f GB of inputs, made in %.1f s" % (N, S, COLS, in_bytes / 1e9, time.perf_counter() - t0),
      flush=True)
eng = mumemto_amd.Engine(0)
for rep in range(3):
    t0 = time.perf_counter()
    m = mumemto_amd.Merged.string_fold(eng, parts, mom, records)
    wall = time.perf_counter() - t0
    st = m.string_fold_stats()
    n_out = m.string_thresh_device()[2]
    print("fold (run %d): %.2f s wall with the uploads; HIP events: split %.2f ms, locate and test %.2f ms, assemble + sort + permute %.2f ms, "
          "thresholds %.2f ms = %.2f TB/s of (4 S + 4) = %d B per position; %d pieces, %d short, %d dropped, %d rows, %d positions" %
          (rep, wall, st["split_ms"], st["locate_ms"], st["assemble_ms"], st["thresholds_ms"],
           (4 * S + 4) * n_out / 1e9 / max(st["thresholds_ms"], 1e-9), 4 * S + 4, st["pieces"], st["dropped_short"], st["dropped_thresh"],
           st["rows"], n_out), flush=True)
    if rep < 2:
        m.close()
# the same workload at the model's size: the device against the closed form, entry by entry
small = workload(N_MODEL, S)
got = mumemto_amd.string_merge_device(*small)
want = merge_mums.string_merge(*small)
print("at %d rows the five results equal the closed form's: %s" % (N_MODEL, all(np.array_equal(g, w) for g, w in zip(got, want))), flush=True)
m.close()
eng.close()
