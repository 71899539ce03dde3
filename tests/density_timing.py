"""GPU box helper: time the add pass of the MEM density (csrc/density_kernels.hip) on the rows of a MEM-mode run of the bench
shape's `-k -1 -f 3` variant (bench.py's collection: synth.collection_sparse, 94 haplotypes x 64 Mbp, divergence 0.001, seed 3;
--haps / --length scale it), in occurrences per second from the HIP events of the pass, best of three:

  spread   the rows as the run left them, bins of 1000 positions and one bin per sequence (W = size)
  piled    the same rows with every start folded into the first 4096 positions of its sequence (a satellite array)
  stacked  every occurrence of a row on the row's first occurrence (document and start): neighbouring lanes share a destination

and the numpy model of tests/densmodel.py on the same rows and box.  The pre-aggregation of the add pass (a workgroup's events
through a table in LDS) is a build-time constant of density_kernels.hpp; for the same figures without it, build a second
library once and name it:

  python tests/density_timing.py --build-variant 0      (where the objects are: mumemto_amd/lib/libmumemto_preagg0.so, DENSITY_PREAGG=0)
  python tests/density_timing.py [--haps N] [--length L]
  python tests/density_timing.py [--haps N] [--length L] --lib mumemto_amd/lib/libmumemto_preagg0.so
"""
import argparse
import os
import subprocess
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import densmodel as M
from mumemto_amd import binding, build, synth

ap = argparse.ArgumentParser()
ap.add_argument("--haps", type=int, default=94)
ap.add_argument("--length", type=int, default=64_000_000)
ap.add_argument("--divergence", type=float, default=0.001)
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--lib", default=None, help="another build of libmumemto.so to time (see --build-variant)")
ap.add_argument("--build-variant", type=int, default=None, metavar="N", help="build libmumemto_preaggN.so with DENSITY_PREAGG=N")
A = ap.parse_args()

if A.build_variant is not None:
    build.build()
    obj = os.path.join(build.OBJ, "density_kernels.preagg%d.o" % A.build_variant)
    subprocess.check_call([build.HIPCC] + build.CXXFLAGS + ["-DDENSITY_PREAGG=%d" % A.build_variant, "-c", os.path.join(build.SRC, "density_kernels.hip"), "-o", obj])
    objs = [obj if s == "density_kernels.hip" else os.path.join(build.OBJ, s + ".o") for s in build.LIB_SOURCES]
    out = os.path.join(build.LIB_DIR, "libmumemto_preagg%d.so" % A.build_variant)
    subprocess.check_call([build.HIPCC, "--offload-arch=" + build.ARCH, "-shared", "-o", out] + objs +
                          ["-Wl,-soname,libmumemto.so", "-Wl,--version-script=" + os.path.join(build.SRC, "libmumemto.map"), "-lz", "-ldl"])
    print("built", out)
    sys.exit(0)

if A.lib:
    binding._LIB = os.path.abspath(A.lib)
import mumemto_amd  # noqa: E402

t0 = time.perf_counter()
bases, lens = synth.collection_sparse(A.haps, A.length, A.divergence, A.seed)
eng = mumemto_amd.Engine(0)
eng.run_partitioned(None, flat=(bases, lens), num_distinct=A.haps - 1, max_doc_freq=3)
lengths, occ_start, starts, docs, _ = eng.rows_mem()
seq_lengths = [int(v) for v in lens]
size, n_occ = max(seq_lengths), len(starts)
print("%s: %d haplotypes x %d bp, -k -1 -f 3: %d rows, %d occurrences (%.1f a row), made and run in %.1f s" %
      (os.path.basename(binding._LIB), A.haps, A.length, len(lengths), n_occ, n_occ / max(len(lengths), 1), time.perf_counter() - t0), flush=True)
counts = np.diff(occ_start.astype(np.int64))
first = occ_start[:-1].astype(np.int64)
cases = (("spread", starts, docs), ("piled", starts % 4096, docs),
         ("stacked", np.repeat(starts[first], counts), np.repeat(docs[first], counts)))
for name, st, dc in cases:
    for W in (1000, size):
        with mumemto_amd.Density(eng, seq_lengths, W) as d:
            best, before = None, 0.0
            for rep in range(3):
                d.add_rows(lengths, occ_start, st, dc)
                ms = d.stats()["add_ms"]
                best, before = (ms - before if best is None else min(best, ms - before)), ms
            d.finish()
            s = d.stats()
            got = d.bins()
        t0 = time.perf_counter()
        want = M.binned(lengths, occ_start, st, dc, seq_lengths, W)
        host = time.perf_counter() - t0
        print("%-7s W = %-9d add pass %8.3f ms = %7.2f G occurrences/s (best of 3); finish %.3f ms over %d bins; cut %d, empty %d; "
              "numpy model %.2f s; three adds equal 3 x the model: %s" %
              (name, W, best, n_occ / best / 1e6, s["finish_ms"], len(seq_lengths) * s["nbins"], s["cut"], s["empty"], host,
               np.array_equal(got, 3 * want)), flush=True)
eng.close()
