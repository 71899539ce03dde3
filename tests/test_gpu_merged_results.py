"""GPU: which results attached to a merged table go when something they read is replaced (MergedRows::table_replaced and
blocks_replaced, csrc/merge_types.hpp), for all five results and all three replacing calls in one place: new blocks take the
inversion calls and the BED records with them and leave coverage and labels, a new table or row order takes everything."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

RESULTS = ("blocks", "calls", "coverage", "bed", "label")


def attached(L, m):
    """the results whose device accessor answers 0; every other one must answer 3 (nothing attached)"""
    a, b = C.c_void_p(), C.c_void_p()
    status = {"blocks": L.mmt_merged_blocks_device(m.h, C.byref(a), C.byref(b)),
              "calls": L.mmt_merged_inversion_calls_device(m.h, C.byref(a)),
              "coverage": L.mmt_merged_coverage_runs_device(m.h, C.byref(a), C.byref(b)),
              "bed": L.mmt_merged_bed_records_device(m.h, C.byref(a), C.byref(b)),
              "label": L.mmt_merged_label_cells_device(m.h, C.byref(a), C.byref(b))}
    assert set(status.values()) <= {0, 3}, status
    return {name for name, rc in status.items() if rc == 0}


def test_what_each_replacing_call_drops():
    import mumemto_amd
    from mumemto_amd import synth
    docs = synth.pangenome(2, 1531, 0.02, seed=5)
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_docs(docs)
        eng.run(merge_metadata=True)                          # (sort_like_direct needs the anchor's suffix ranks)
        n, nd, a, b, c = eng.rows_mum_device()
        assert n > 3 and nd == 2
        contigs = ([["x"], ["y"]], [[10000], [10000]])
        with mumemto_amd.Merged.from_device(eng, n, nd, a, b, c) as m:
            assert attached(eng.L, m) == set()

            def attach_all():
                blk = m.collinear(1000, 0)
                m.inversions()
                m.coverage([10000, 10000])
                assert m.bed(contigs, None, 0) > 0 and m.label(contigs) > 0
                assert attached(eng.L, m) == set(RESULTS)
                return blk

            blk = attach_all()
            assert len(blk)
            m.set_blocks(blk)                                 # new blocks: what reads the blocks goes, what reads the table stays
            assert attached(eng.L, m) == {"blocks", "coverage", "label"}
            attach_all()
            m.collinear(1000, 0)                              # a filtered, sorted table and its blocks
            assert attached(eng.L, m) == {"blocks"}
            attach_all()
            assert eng.L.mmt_merged_sort_like_direct(eng.h, m.h) == 0      # a new row order
            assert attached(eng.L, m) == set()
            attach_all()                                      # and everything can be had again
    finally:
        eng.close()
