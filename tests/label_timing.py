"""GPU box helper: time the contig labels on a seeded table (default 2 M rows x 94 columns, starts ascending in every column, a
twentieth of the cells absent, 300 contigs per sequence) stage by stage: the lookup, then the text with numbers and with names,
written in pieces to /dev/null.  Where the reference's tree is mounted, its own tool is timed on a 1/100 sample of the table
(with `reference` as the only argument: that alone, no GPU needed).

  python tests/label_timing.py [rows] [columns] [contigs per sequence]
  python tests/label_timing.py reference [rows] [columns] [contigs per sequence]
"""
import contextlib
import io
import os
import sys
import tempfile
import time
import types

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import numpy as np
import labelmodel as M

REFERENCE = "/root/reference/mumemto"
argv = sys.argv[1:]
ONLY_REFERENCE = bool(argv) and argv[0] == "reference"
argv = argv[1:] if ONLY_REFERENCE else argv
N = int(argv[0]) if len(argv) > 0 else 2_000_000
ND = int(argv[1]) if len(argv) > 1 else 94
NC = int(argv[2]) if len(argv) > 2 else 300


def time_reference(lengths, starts, strands, contigs):
    """the reference's tool on the first hundredth of the rows, through files as it wants them"""
    from mumemto_amd import mumsio
    pkg = types.ModuleType("mumemto")
    pkg.__path__ = [REFERENCE]
    sys.modules["mumemto"] = pkg
    from mumemto import get_sequence_info as ref_label
    k = max(N // 100, 1)
    with tempfile.TemporaryDirectory() as tmp:
        src, lens = os.path.join(tmp, "sample.mums"), os.path.join(tmp, "sample.lengths")
        mumsio.write_mums(src, lengths[:k], starts[:k], strands[:k])
        with open(lens, "w") as f:
            for c, (names, seq) in enumerate(zip(*contigs)):
                f.write("/g/%d.fa * %d\n" % (c, sum(seq)))
                for name, v in zip(names, seq):
                    f.write("/g/%d.fa %s %d\n" % (c, name, v))
        for flags in ([], ["-n"]):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                ref_label.main(ref_label.parse_arguments(["-m", src, "-l", lens, "-o", os.path.join(tmp, "out.mums")] + flags))
            wall = time.perf_counter() - t0
            same = open(os.path.join(tmp, "out.mums"), "rb").read() == M.label(lengths[:k], starts[:k], strands[:k], contigs, None, bool(flags))[2]
            print("reference tool %s on %d rows x %d columns (1/100 of the table, with reading its .mums file): %.2f s wall, i.e. "
                  "%.0f s for the table; bytes equal to the model: %s" % (" ".join(flags) or "(numbers)", k, ND, wall, wall * N / k, same),
                  flush=True)


t0 = time.perf_counter()
lengths, starts, strands, totals = M.make_rows(1, N, ND, absent=0.05)
contigs = M.make_contigs(3, totals, [NC] * ND)
print("table: %d rows x %d columns, %.2f GB of starts, %d contigs per sequence, made in %.1f s" %
      (N, ND, starts.nbytes / 1e9, NC, time.perf_counter() - t0), flush=True)
if not ONLY_REFERENCE:
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    m = mumemto_amd.Merged.from_rows(eng, lengths, starts, strands)
    for names in (False, True):
        for rep in range(2):
            t0 = time.perf_counter()
            n_bytes = m.label(contigs, names)
            wall = time.perf_counter() - t0
            s = m.label_stats()
            print("label%s (run %d): %.1f ms wall; HIP events: lookup %.2f ms (%.1f GB/s of 20 B a cell), measure + scan %.2f ms; "
                  "%d cells, %d absent, %d columns from HBM, %.2f GB of text" %
                  (", names" if names else "", rep, wall * 1e3, s["lookup_ms"], 20e-6 * s["cells"] / max(s["lookup_ms"], 1e-9),
                   s["measure_ms"], s["cells"], s["absent"], s["hbm_columns"], n_bytes / 1e9), flush=True)
        before = m.label_stats()
        t0 = time.perf_counter()
        m.write_label("/dev/null")
        wall = time.perf_counter() - t0
        s = m.label_stats()
        write_ms = s["write_ms"] - before["write_ms"]
        print("text%s to /dev/null in pieces: %.1f ms wall; HIP events: measure + scan %.2f, write %.2f ms (%.1f GB/s of text), copies to "
              "the host + wait %.2f ms" % (", names" if names else "", wall * 1e3, s["measure_ms"] - before["measure_ms"], write_ms,
                                          s["text_bytes"] / 1e6 / max(write_ms, 1e-9), s["copy_ms"] - before["copy_ms"]), flush=True)
    k = min(N, 20000)
    contig, rel = m.label_cells()
    want = M.cells(starts[:k], contigs[1])
    print("the first %d rows equal the numpy model: %s" % (k, np.array_equal(contig[:k], want[0]) and np.array_equal(rel[:k], want[1])),
          flush=True)
    m.close()
    eng.close()
if os.path.isdir(REFERENCE):
    time_reference(lengths, starts, strands, contigs)
else:
    print("the reference's tree is not mounted here: its tool is not timed", flush=True)
