"""Inputs of the string fold (mumemto_amd/csrc/string_fold.cpp) and the checks of its outputs against the closed form,
mumemto_amd/merge_mums.py string_merge.  No GPU is needed here: the generator, a loop restatement of the closed form that
says WHY every piece was kept or dropped (trace), and the check functions are used by tests/test_string_fold_host.py on the
model alone and by tests/test_gpu_string_fold.py on the device.

The fold is arithmetic on tables, so the inputs are not real MUMs; they satisfy what the fold requires of its inputs:
partitions in ascending order of column 0 without absent starts, threshold tables of sum(length + 1) entries, one record per
partition row in the MUMs-of-MUMs' collection with the last record cut short (extract_mums truncates the row that touches the
end of the first document: 20 against 40 in tests/golden/string_merge/two_by_two)."""
import numpy as np

MIN_SEGMENT = 20
TILE = 2048                      # sk::THRESH_TILE: output positions of one workgroup tile of the threshold pass
MAX_ROWS, LDS_BYTES = 128, 48 * 1024     # sk::THRESH_MAX_ROWS, sk::THRESH_LDS_BYTES


def rows_at_once(S):
    """sk::thresholds_rows_at_once: the rows of a tile the threshold pass holds in LDS at a time; a tile with more takes rounds"""
    R = MAX_ROWS
    while R and (R + 1) * 8 + R * S * 16 + R * 4 + R * S > LDS_BYTES:
        R >>= 1
    return R


def most_rows_in_a_tile(lengths):
    begins = np.cumsum(lengths.astype(np.int64) + 1) - lengths - 1
    return int(np.bincount(begins // TILE).max()) if len(lengths) else 0


# ---- building blocks ------------------------------------------------------------------------------------------------------
def make_part(rng, lengths, n_cols, base=0, th_max=9, zero_rate=0.0, minus_rate=0.3, gap=40):
    """-> ((lengths, starts, strands, thresh, thresh_rev), records): rows one after the other in column 0, the other columns
    anywhere; thresholds 1..th_max (0 with zero_rate) and 0 behind every row; the last record half as long as its row"""
    lengths = np.asarray(lengths, np.uint32)
    n = len(lengths)
    starts = base + rng.integers(0, 1 << 20, (n, n_cols)).astype(np.int64)
    step = lengths.astype(np.int64) + rng.integers(0, gap + 1, n)
    starts[:, 0] = base + np.cumsum(step) - step
    strands = rng.random((n, n_cols)) >= minus_rate
    ends = np.cumsum(lengths.astype(np.int64) + 1)
    tables = []
    for _ in range(2):
        th = rng.integers(1, th_max + 1, int(ends[-1]) if n else 0).astype(np.uint16)
        th[rng.random(len(th)) < zero_rate] = 0
        th[ends - 1] = 0
        tables.append(th)
    records = lengths.astype(np.int64) + 1
    if n:
        records[-1] = max(1, records[-1] // 2)
    return (lengths, starts, strands, tables[0], tables[1]), records


def rec_begin(records):
    return np.concatenate(([0], np.cumsum(records)))


def mom_rows(records, rows):
    """rows: (length, [(record, offset, forward) per collection]) -> (lengths, starts, strands) of the MUMs of MUMs"""
    begin = [rec_begin(r) for r in records]
    S = len(records)
    lengths = np.array([r[0] for r in rows], np.uint32)
    starts = np.array([[begin[i][g] + o for i, (g, o, _) in enumerate(r[1])] for r in rows], np.int64).reshape(len(rows), S)
    strands = np.array([[f for _, _, f in r[1]] for r in rows], bool).reshape(len(rows), S)
    return lengths, starts, strands


# ---- why a piece was kept or dropped: the closed form, piece by piece --------------------------------------------------------
def trace(parts, mom, mom_records):
    """one dict per piece of every row of mom, in order: row, k (piece of the row), of (pieces of the row), length, short (dropped as
    shorter than MIN_SEGMENT), and for the others per partition: exists (the record), last (it is the last record), th, strand of
    the match, minus (the located row has a `-` cell), ok, clamped_low / clamped_high (an index of the row's thresholds lies before /
    behind the table); kept = every partition ok"""
    S = len(parts)
    ends = [np.cumsum(r) for r in mom_records]
    term = ends[0] - 1
    lengths, starts, strands = mom
    out = []
    for r in range(len(lengths)):
        s0, L = int(starts[r, 0]), int(lengths[r])
        cuts = [int(t) for t in term if s0 <= t < s0 + L]
        edges = [0] + [t - s0 for t in cuts] + [L]
        for k in range(len(cuts) + 1):
            left = 0 if k == 0 else edges[k] + 1
            end = edges[k + 1]
            p = dict(row=r, k=k, of=len(cuts) + 1, length=end - left, short=end - left < MIN_SEGMENT and len(cuts) > 0, parts=[])
            out.append(p)
            if p["short"]:
                p["kept"] = False
                continue
            for i in range(S):
                v = int(starts[r, i]) + (left if strands[r, i] else L - end)
                rec = int(np.searchsorted(ends[i], v, "right"))
                exists = rec < len(ends[i])
                th = int(parts[i][3][min(max(v, 0), len(parts[i][3]) - 1)]) if len(parts[i][3]) else 0
                rc = min(rec, len(ends[i]) - 1)
                rev = int(ends[i][rc - 1] if rc > 0 else 0) + int(ends[i][rc]) - v - p["length"] - 1 if len(ends[i]) else 0
                T = len(parts[i][3])                                  # the row's thresholds: [v, v + length) and [rev, rev + length)
                p["parts"].append(dict(exists=exists, last=exists and rec == len(ends[i]) - 1, th=th, forward=bool(strands[r, i]),
                                       minus=bool(exists and not parts[i][2][rc].all()), ok=exists and th != 0 and p["length"] > th,
                                       clamped_low=min(v, rev) < 0, clamped_high=max(v, rev) + p["length"] > T))
            p["kept"] = all(q["ok"] for q in p["parts"])
    return out


def counts(tr):
    """what mmt_merged_string_fold_stats reports in [4..7]: pieces cut, dropped short, dropped by a partition, rows"""
    short = sum(p["short"] for p in tr)
    rows = sum(p["kept"] for p in tr)
    return dict(pieces=len(tr), dropped_short=short, dropped_thresh=len(tr) - short - rows, rows=rows)


# ---- named cases --------------------------------------------------------------------------------------------------------------
# name -> (build(rng) -> (parts, mom, mom_records), reached(trace, parts, want) -> bool: the model met the boundary the case is named for)
def _two_parts(rng, lengths, cols=(2, 2), **kw):
    made = [make_part(rng, lengths, c, **kw) for c in cols]
    return [m[0] for m in made], [m[1] for m in made]


def case_cut_0_1_3(rng):
    parts, records = _two_parts(rng, [30] * 8)
    rows = [(24, [(0, 3, True), (1, 2, True)]),                       # inside a record
            (25 + 1 + 22, [(1, 5, True), (2, 0, True)]),              # one `#`: 25 + 22
            (22 + 1 + 30 + 1 + 30 + 1 + 21, [(2, 8, True), (3, 0, False)])]   # three: 22, 30, 30, 21
    return parts, mom_rows(records, rows), records


def case_piece_19_20(rng):
    parts, records = _two_parts(rng, [30] * 6)
    rows = [(19 + 1 + 20, [(1, 11, True), (2, 0, True)]), (20 + 1 + 19, [(3, 10, True), (0, 0, True)])]
    return parts, mom_rows(records, rows), records


def case_short_single(rng):
    parts, records = _two_parts(rng, [30] * 4, th_max=5)
    rows = [(7, [(1, 2, True), (2, 4, True)]), (19, [(2, 1, True), (0, 3, False)])]
    return parts, mom_rows(records, rows), records


def case_last_record(rng):
    parts, records = _two_parts(rng, [40] * 4)                        # the last records: 20 of 41
    rows = [(12, [(3, 2, True), (3, 4, True)]),                       # in the truncated last record of both
            (12, [(1, 2, True), (3, 25, True)]),                      # beyond the last record of collection 1: dropped
            (25, [(0, 1, True), (1, 1, True)])]
    return parts, mom_rows(records, rows), records


def case_thresh_zero(rng):
    parts, records = _two_parts(rng, [30] * 4)
    parts[1][3][rec_begin(records[1])[2] + 4] = 0
    rows = [(22, [(0, 1, True), (2, 4, True)]), (22, [(1, 1, True), (2, 5, True)])]
    return parts, mom_rows(records, rows), records


def case_len_eq_th(rng):
    parts, records = _two_parts(rng, [40] * 4)
    at = rec_begin(records[0])
    parts[0][3][at[1] + 3] = 24
    parts[0][3][at[2] + 3] = 24
    rows = [(24, [(1, 3, True), (0, 2, True)]), (25, [(2, 3, True), (1, 2, True)])]     # == th: dropped; th + 1: kept
    return parts, mom_rows(records, rows), records


def case_four_signs(rng):
    parts, records = _two_parts(rng, [40] * 8, cols=(2, 3), minus_rate=0.0)
    for p in parts:
        p[2][::2] = False                                             # `-` cells in every other row of both partitions
    rows = [(25, [(g, 2, f0), (h, 3, f1)]) for g, h, f0, f1 in
            [(0, 0, True, True), (1, 1, True, False), (2, 3, False, True), (3, 2, False, False),
             (4, 5, True, False), (5, 4, False, True), (6, 6, False, False)]]
    return parts, mom_rows(records, rows), records


def _whole_rows(rng, parts, records, n, length=None):
    rows = []
    for g in range(n):
        L = int(parts[0][0][g]) if length is None else length
        rows.append((L, [(g, 0, True)] + [(g, 0, bool(rng.integers(0, 2))) for _ in parts[1:]]))
    return mom_rows(records, rows)


def case_cols_1_3(rng):
    parts, records = _two_parts(rng, [35] * 6, cols=(1, 3))
    return parts, _whole_rows(rng, parts, records, 5), records


def case_cols_2_2_2(rng):
    parts, records = _two_parts(rng, [35] * 6, cols=(2, 2, 2))
    return parts, _whole_rows(rng, parts, records, 5), records


def case_wide_starts(rng):
    made = [make_part(rng, [33] * 6, 2, base=b) for b in ((1 << 32) + 12345, (1 << 39) + 777)]
    parts, records = [m[0] for m in made], [m[1] for m in made]
    return parts, _whole_rows(rng, parts, records, 5), records


def case_equal_col0(rng):
    parts, records = _two_parts(rng, [30] * 6)
    parts[0][1][2, 0] = parts[0][1][1, 0]                             # rows 1 and 2 of partition 0 begin at the same place
    parts[0][1][3, 0] = parts[0][1][1, 0]
    rows = [(30, [(g, 0, True), (h, 0, True)]) for g, h in [(3, 0), (2, 1), (1, 2), (0, 3)]]
    mom = mom_rows(records, rows)
    order = np.argsort(mom[1][:, 1], kind="stable")                   # any order of mom's rows is legal: not that of column 0
    return parts, tuple(a[order] for a in mom), records


def case_negative_col0(rng):
    """starts are signed: rows of column 0 on either side of 0 (never -1) come out in signed order"""
    parts, records = _two_parts(rng, [30] * 8)
    col0 = parts[0][1][:, 0]
    col0 -= col0[4] + 7
    col0[col0 == -1] = -2
    return parts, _whole_rows(rng, parts, records, 7), records


def case_clamped(rng):
    """np.take(mode="clip") is kept: a piece that runs over the end of its record reads thresholds before the table's first entry
    (the reverse table, in the first record) and behind its last (in the truncated last record)"""
    parts, records = _two_parts(rng, [40] * 4)                        # records 41, 41, 41, 20; tables of 164
    rows = [(25, [(1, 2, True), (3, 18, True)]),                      # 141 + 25 > 164
            (25, [(2, 3, True), (0, 30, True)]),                      # the reverse table from 41 - 30 - 25 - 1 = -15
            (25, [(0, 4, True), (3, 17, False)]),
            (25, [(1, 9, True), (2, 1, True)])]
    return parts, mom_rows(records, rows), records


def case_many_short_rows(rng):
    """one-piece rows of 2 .. 6 over thresholds of 1: some 400 rows in a tile, more than the pass holds at a time"""
    parts, records = _two_parts(rng, rng.integers(2, 7, 1500), th_max=1)
    return parts, _whole_rows(rng, parts, records, 1499), records


def case_many_partitions(rng):
    """24 partitions: the pass holds 64 rows at a time, and rows of 8 .. 14 put some 170 into a tile"""
    parts, records = _two_parts(rng, rng.integers(8, 15, 500), cols=(1,) * 24, th_max=1)
    return parts, _whole_rows(rng, parts, records, 499), records


def case_tile_edges(rng):
    lengths = [20, 63, 64, 65, 2 * TILE + 517, 20, 63, 64, 65, TILE - 1, TILE, 300, 40]
    parts, records = _two_parts(rng, lengths, th_max=19)
    return parts, _whole_rows(rng, parts, records, len(lengths) - 1), records


def case_empty(rng):
    parts, records = _two_parts(rng, [30] * 4, zero_rate=1.0)
    return parts, _whole_rows(rng, parts, records, 3), records


def _kept(tr):
    return [p for p in tr if p["kept"]]


def _dropped_by(tr, why):
    return [p for p in tr if not p["short"] and not p["kept"] and any(why(q) for q in p["parts"])]


NAMED = {
    "cut_0_1_3": (case_cut_0_1_3, lambda tr, parts, want: {p["of"] for p in tr} >= {1, 2, 4} and len(_kept(tr)) >= 3),
    "piece_19_20": (case_piece_19_20, lambda tr, parts, want: any(p["short"] and p["length"] == 19 for p in tr)
                    and any(p["kept"] and p["length"] == 20 and p["of"] == 2 for p in tr)),
    "short_single": (case_short_single, lambda tr, parts, want: any(p["kept"] and p["of"] == 1 and p["length"] < MIN_SEGMENT for p in tr)),
    "last_record": (case_last_record, lambda tr, parts, want: any(p["kept"] and all(q["last"] for q in p["parts"]) for p in tr)
                    and bool(_dropped_by(tr, lambda q: not q["exists"]))),
    "thresh_zero": (case_thresh_zero, lambda tr, parts, want: bool(_dropped_by(tr, lambda q: q["exists"] and q["th"] == 0)) and bool(_kept(tr))),
    "len_eq_th": (case_len_eq_th, lambda tr, parts, want: any(not p["kept"] and any(q["th"] == p["length"] for q in p["parts"]) for p in tr)
                  and any(p["kept"] and any(q["th"] + 1 == p["length"] for q in p["parts"]) for p in tr)),
    "four_signs": (case_four_signs, lambda tr, parts, want: {(q["forward"], q["minus"]) for p in _kept(tr) for q in p["parts"]}
                   == {(True, True), (True, False), (False, True), (False, False)}),
    "cols_1_3": (case_cols_1_3, lambda tr, parts, want: [p[1].shape[1] for p in parts] == [1, 3] and want[1].shape[1] == 4 and len(want[0]) > 0),
    "cols_2_2_2": (case_cols_2_2_2, lambda tr, parts, want: [p[1].shape[1] for p in parts] == [2, 2, 2] and want[1].shape[1] == 6
                   and len(want[0]) > 0),
    "wide_starts": (case_wide_starts, lambda tr, parts, want: len(want[0]) > 0 and (want[1][:, :2] > 1 << 32).all()
                    and (want[1][:, :2] < 1 << 39).all() and (want[1][:, 2:] > 1 << 39).all()),
    "equal_col0": (case_equal_col0, lambda tr, parts, want: len(want[0]) >= 3 and (np.diff(want[1][:, 0]) == 0).sum() >= 2
                   and len(np.unique(want[1][:, 2])) == len(want[0])),
    "negative_col0": (case_negative_col0, lambda tr, parts, want: (want[1][:, 0] < 0).sum() >= 2 and (want[1][:, 0] > 0).sum() >= 2),
    "clamped": (case_clamped, lambda tr, parts, want: any(q["clamped_low"] for p in _kept(tr) for q in p["parts"])
                and any(q["clamped_high"] for p in _kept(tr) for q in p["parts"])
                and any(not q["clamped_low"] and not q["clamped_high"] for p in _kept(tr) for q in p["parts"])),
    "many_short_rows": (case_many_short_rows, lambda tr, parts, want: rows_at_once(2) == MAX_ROWS and len(want[3]) > 2 * TILE
                        and most_rows_in_a_tile(want[0]) > 2 * MAX_ROWS),
    "many_partitions": (case_many_partitions, lambda tr, parts, want: len(parts) == 24 and 0 < rows_at_once(24) < MAX_ROWS
                        and len(want[3]) > 2 * TILE and most_rows_in_a_tile(want[0]) > 2 * rows_at_once(24)),
    "tile_edges": (case_tile_edges, lambda tr, parts, want: set(want[0].tolist()) >= {20, 63, 64, 65, TILE - 1, TILE, 2 * TILE + 517}),
    "empty": (case_empty, lambda tr, parts, want: len(tr) > 0 and not _kept(tr) and len(want[0]) == 0 and len(want[3]) == 0 == len(want[4])
              and want[1].shape == (0, 4)),
}


def named_case(name):
    return NAMED[name][0](np.random.default_rng(sorted(NAMED).index(name) + 1000))


# ---- the seeded sweep ----------------------------------------------------------------------------------------------------------
def random_case(seed):
    """2 - 4 partitions of 1 - 3 columns and 40 - 400 rows; rows of mom inside one record of collection 0 or across one to three
    `#`, forward or reversed in the other collections, there anywhere in a record (so a piece may run over its record's end:
    the offsets go negative and the threshold indices are clamped, as in the closed form)"""
    rng = np.random.default_rng(seed)
    S = int(rng.integers(2, 5))
    made = []
    for _ in range(S):
        n = int(rng.integers(40, 401))
        lengths = rng.integers(20, 200, n)
        lengths[rng.random(n) < 0.02] = int(rng.integers(1000, 3 * TILE))
        made.append(make_part(rng, lengths, int(rng.integers(1, 4)), base=int(rng.integers(0, 2)) * ((1 << 33) + 5), th_max=12, zero_rate=0.02))
    parts, records = [m[0] for m in made], [m[1] for m in made]
    begin = [rec_begin(r) for r in records]
    rows = []
    for _ in range(int(rng.integers(30, 600))):
        n0 = len(records[0])
        span = int(rng.choice([0, 0, 0, 0, 1, 3]))
        g = int(rng.integers(0, max(1, n0 - span)))
        o = int(rng.integers(0, max(1, records[0][g] - 21)))
        h = min(g + span, n0 - 1)
        stop = int(begin[0][h]) + (int(rng.integers(min(20, records[0][h] - 1), records[0][h])) if h > g else int(records[0][g]) - 1)
        L = max(1, stop - (int(begin[0][g]) + o))
        cells = [(g, o, True)]
        for i in range(1, S):
            gi = int(rng.integers(0, len(records[i])))
            cells.append((gi, int(rng.integers(0, max(1, records[i][gi] - 1))), bool(rng.random() < 0.7)))
        rows.append((L, cells))
    return parts, mom_rows(records, rows), records


SWEEP_SEEDS = list(range(7000, 7020))


# ---- the checks of an output against the closed form's ---------------------------------------------------------------------------
FIELDS = ("lengths", "starts", "strands", "thresh", "thresh_rev")
DTYPES = (np.uint32, np.int64, np.bool_, np.uint16, np.uint16)


def check_fold(got, want, what=""):
    """the five results of a fold against the closed form's: dtype, shape and every entry"""
    assert len(got) == len(want) == 5, what
    for name, dtype, g, w in zip(FIELDS, DTYPES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == dtype, "%s %s: dtype %s" % (what, name, g.dtype)
        assert g.shape == w.shape, "%s %s: shape %s, the model's %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = tuple(int(x[0]) for x in np.nonzero(g != w))
            raise AssertionError("%s %s: %d entries differ, the first at %s: %s, the model's %s" % (what, name, int((g != w).sum()), at, g[at], w[at]))


def check_counts(stats, tr, what=""):
    want = counts(tr)
    for key, v in want.items():
        assert stats[key] == v, "%s %s: %d, the model's %d" % (what, key, stats[key], v)
