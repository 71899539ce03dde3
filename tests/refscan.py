"""The reference's own match scan as a checker (oracle/_ref/mem_finder_ref, built by oracle/Makefile target `ref` from
include/mem_finder.hpp + include/read_arrays.hpp and our driver oracle/_ref_drivers/mem_finder_driver.cpp).

write_arrays() writes a stream in the `-a` format (40-bit SA / LCP, one BWT byte per entry) plus the per-document text
lengths; run() streams every entry of those files through mem_finder and returns what mem_finder::close() wrote;
oracle_files() gives the same files from the C restatement (oracle/mumemto_oracle.c) for the same stream."""
import os
import subprocess

import numpy as np

import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "mem_finder_ref")
EXTS = (".mums", ".mems", ".bumbl", ".thresh", ".thresh_rev", ".athresh")


def available():
    return os.path.exists(BIN)


def put40(values):
    """int64 array -> bytes of 5-byte little-endian entries."""
    v = np.ascontiguousarray(values, dtype="<u8")
    if len(v) and int(v.max()) >> 40:
        raise ValueError("entry beyond 40 bits")
    return v.view(np.uint8).reshape(-1, 8)[:, :5].tobytes()


def write_arrays(prefix, sa, lcp, bwt, doc_text_len):
    """The -a files PREFIX.sa / .lcp / .bwt, and PREFIX.doclens (one document length in the text per line)."""
    with open(prefix + ".sa", "wb") as f:
        f.write(put40(sa))
    with open(prefix + ".lcp", "wb") as f:
        f.write(put40(lcp))
    with open(prefix + ".bwt", "wb") as f:
        f.write(np.ascontiguousarray(bwt, np.uint8).tobytes())
    with open(prefix + ".doclens", "w") as f:
        f.write("".join("%d\n" % int(x) for x in doc_text_len))


def run_files(prefix, out, doc_text_len, min_len, num_distinct, max_doc_freq=1, max_total_freq=0, revcomp=True,
              binary=False, merge=False, anchor_merge=False, timeout=120):
    """Runs the reference scan over the -a files under `prefix` (PREFIX.doclens written if absent) -> {ext: bytes}."""
    if not os.path.exists(prefix + ".doclens"):
        with open(prefix + ".doclens", "w") as f:
            f.write("".join("%d\n" % int(x) for x in doc_text_len))
    args = [BIN, prefix, out, min_len, num_distinct, max_doc_freq, max_total_freq, int(revcomp), int(binary), int(merge),
            int(anchor_merge)]
    r = subprocess.run([str(a) for a in args], capture_output=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("mem_finder_ref exited %d: %s" % (r.returncode, r.stderr.decode(errors="replace")[-400:]))
    got = {}
    for ext in EXTS:
        if os.path.exists(out + ext):
            with open(out + ext, "rb") as f:
                got[ext] = f.read()
    return got


def run(sa, lcp, bwt, doc_text_len, workdir, min_len=20, num_distinct=0, max_doc_freq=1, max_total_freq=0, revcomp=True,
        binary=False, merge=False, anchor_merge=False, tag="s", timeout=120):
    """Writes the stream under workdir and runs the reference scan over it -> {ext: bytes}."""
    prefix = os.path.join(str(workdir), tag + "_in")
    out = os.path.join(str(workdir), tag + "_out")
    for ext in EXTS:
        if os.path.exists(out + ext):
            os.remove(out + ext)
    write_arrays(prefix, sa, lcp, bwt, doc_text_len)
    nd = num_distinct if num_distinct else len(doc_text_len)
    return run_files(prefix, out, doc_text_len, min_len, nd, max_doc_freq, max_total_freq, revcomp, binary, merge,
                     anchor_merge, timeout)


def oracle_result(sa, lcp, bwt, doc_text_len, min_len=20, num_distinct=0, max_doc_freq=1, max_total_freq=0, revcomp=True,
                  merge=False):
    doc_start = np.zeros(len(doc_text_len) + 1, np.int64)
    doc_start[1:] = np.cumsum(np.asarray(doc_text_len, np.int64))
    return O.scan(np.ascontiguousarray(sa, np.int64), np.ascontiguousarray(lcp, np.int64),
                  np.ascontiguousarray(bwt, np.uint8), doc_start, min_len=min_len, num_distinct=num_distinct,
                  max_doc_freq=max_doc_freq, max_total_freq=max_total_freq, revcomp=revcomp, merge=merge)


def oracle_files(res, doc_text_len, revcomp=True, binary=False, merge=False, anchor_merge=False):
    """The files mem_finder::close() writes, from an oracle ScanResult (mem_finder.hpp:97-158)."""
    out = {}
    if not res.mummode:
        out[".mems"] = res.text()
    elif binary:
        out[".bumbl"] = res.bumbl()
    else:
        out[".mums"] = res.text()
    half0 = int(doc_text_len[0]) // (2 if revcomp else 1)
    if anchor_merge:
        out[".athresh"] = res.thresh()[:half0].tobytes()
    elif merge:
        out[".thresh"] = res.thresh_file(False).tobytes()
        out[".thresh_rev"] = res.thresh_file(True).tobytes()
    return out


def doc_text_lengths(docs, revcomp=True):
    """Per-document length in the text: (revcomp ? 2 : 1) * (bases + 1)."""
    return [(2 if revcomp else 1) * (sum(len(r) for r in d) + 1) for d in docs]
