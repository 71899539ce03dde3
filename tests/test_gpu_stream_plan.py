"""The PLAN of the bucket-wise producer's stream loops (guided.cpp), not only their bytes: how many passes over the text, batches
and windows a run takes, how many stream entries it produces and where the ranks' shares are cut.  The figures below were
recorded from the commit before the loops got their one share cut, batch feeder and window hand-off; a change of the collection
protocol that still gives the oracle's bytes (a count that is repeated, a look-ahead that is lost, another pass rule) shows here.

With MMT_GUIDED_BATCH set the capacities do not depend on the free device memory, so the figures are the same on every device.
The expansion loop is reached with MUMEMTO_EXPAND=1: a producer that is named "guided" stays the plain one otherwise (pfp.cpp),
whatever the collection -- none of the parametrisations of test_bucket_wise_producer_on_many_copies_equals_the_oracle expands
by itself, so the first and smallest of them is the input."""
import pytest

import pyoracle as O
from mumemto_amd import synth
from test_gpu_packed import packed_env
from test_gpu_realistic import _gap_docs

pytestmark = pytest.mark.gpu

MODES = {"mum": dict(), "mem": dict(num_distinct=8, max_doc_freq=3, max_total_freq=27)}

# Recorded on commit 4ed49e0 ("Pin the anchor fold to the reference's anchor_merge on built partitions"), the parent of the
# commit that introduced this file, by tests/test_gpu_stream_plan.py::observe itself; never from the code under test.
# key: loop / mode / MMT_GUIDED_STAGE / shard -> (run_slices, text_passes, batches, staged), entries, windows, sort_pieces
EXPECTED = {
    'plain/mum/stage0/0of1': ((0, 26, 26, False), 720012, 26, [(0, 720012)]),
    'plain/mum/stage0/0of3': ((0, 9, 9, False), 241936, 9, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mum/stage0/1of3': ((0, 9, 9, False), 240149, 9, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mum/stage0/2of3': ((0, 9, 9, False), 237927, 9, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mum/stage1/0of1': ((0, 7, 31, True), 720012, 31, [(0, 720012)]),
    'plain/mum/stage1/0of3': ((0, 3, 11, True), 241936, 11, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mum/stage1/1of3': ((0, 3, 11, True), 240149, 11, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mum/stage1/2of3': ((0, 2, 10, True), 237927, 10, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mem/stage0/0of1': ((0, 26, 26, False), 720012, 26, [(0, 720012)]),
    'plain/mem/stage0/0of3': ((0, 9, 9, False), 241936, 9, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mem/stage0/1of3': ((0, 9, 9, False), 240149, 9, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mem/stage0/2of3': ((0, 9, 9, False), 237927, 9, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mem/stage1/0of1': ((0, 7, 31, True), 720012, 31, [(0, 720012)]),
    'plain/mem/stage1/0of3': ((0, 3, 11, True), 241936, 11, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mem/stage1/1of3': ((0, 3, 11, True), 240149, 11, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'plain/mem/stage1/2of3': ((0, 2, 10, True), 237927, 10, [(0, 241936), (241936, 240149), (482085, 237927)]),
    'expand/mum/stage0/0of1': ((0, 9, 9, False), 721588, 27, [(0, 721588)]),
    'expand/mum/stage0/0of2': ((0, 5, 5, False), 360806, 14, [(0, 360806), (360806, 360782)]),
    'expand/mum/stage0/1of2': ((0, 5, 5, False), 360782, 14, [(0, 360806), (360806, 360782)]),
    'expand/mum/stage1/0of1': ((0, 3, 11, True), 721588, 29, [(0, 721588)]),
    'expand/mum/stage1/0of2': ((0, 2, 6, True), 360806, 15, [(0, 360806), (360806, 360782)]),
    'expand/mum/stage1/1of2': ((0, 2, 5, True), 360782, 14, [(0, 360806), (360806, 360782)]),
    'slices/mem/0of1': ((58, 40, 30, True), 452860, 88, [(0, 452860)]),
}

_cache = {}


def _plain_docs():
    return synth.pangenome(9, 40000, 0.01, seed=41, indel_rate=0.0005, inversion=(4, 3000, 9000))


def _copies_docs():
    haps, length = 12, 30_000
    return synth.pangenome(haps, length, 0.004, seed=haps, indel_rate=0.001, tandem=(1, 500, 700, 4))


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def observe(docs, producer, kw, shard, count, expanded):
    """one run of a fresh engine: (the plan's figures, the bytes)"""
    import mumemto_amd
    eng = mumemto_amd.Engine(0)
    try:
        eng.set_producer("guided", *producer)
        eng.set_scan_shard(shard, count)
        eng.set_docs(docs)
        eng.run(**kw)
        assert eng.producer_used() == "guided" and eng.producer_expanded() == expanded
        st, ss = eng.producer_stats(), eng.stream_stats()
        plan = ((st["run_slices"], st["text_passes"], st["batches"], st["staged"]), ss["entries"], ss["windows"],
                eng.sort_pieces())
        return plan, eng.output_text()
    finally:
        eng.close()


def check(key, plan):
    print("    %r: %r," % (key, plan))            # (pytest -s: the figures before they are asserted)
    assert plan == EXPECTED[key], key


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("mode", ["mum", "mem"])
def test_plan_of_the_plain_loop(mode, stage):
    docs = _once("plain", _plain_docs)
    want = _once(("plain", mode), lambda: O.run(docs, **MODES[mode]).text())
    with packed_env(MMT_GUIDED_BATCH=30000, MMT_SCAN_RANGE=16384, MMT_GUIDED_STAGE=stage):
        plan, text = observe(docs, (), MODES[mode], 0, 1, False)
        check("plain/%s/stage%d/0of1" % (mode, stage), plan)
        assert text == want
        pieces = b""
        for r in range(3):
            plan, text = observe(docs, (), MODES[mode], r, 3, False)
            check("plain/%s/stage%d/%dof3" % (mode, stage, r), plan)
            pieces += text
        assert pieces == want


@pytest.mark.parametrize("stage", [0, 1])
def test_plan_of_the_expansion_loop(stage):
    docs = _once("copies", _copies_docs)
    want = _once(("copies", "mum"), lambda: O.run(docs).text())
    with packed_env(MMT_GUIDED_BATCH=30000, MMT_SCAN_RANGE=16384, MMT_GUIDED_STAGE=stage, MUMEMTO_EXPAND=1):
        plan, text = observe(docs, (10, 30), {}, 0, 1, True)
        check("expand/mum/stage%d/0of1" % stage, plan)
        assert text == want
        pieces = b""
        for r in range(2):
            plan, text = observe(docs, (10, 30), {}, r, 2, True)
            check("expand/mum/stage%d/%dof2" % (stage, r), plan)
            pieces += text
        assert pieces == want


def test_plan_of_a_run_bin_in_slices():
    seed, limit, wp = 1, "3000", (6, 16)           # the smallest case of test_bins_of_one_repeated_symbol_are_produced_in_slices
    docs = _gap_docs(seed)
    kw = dict(num_distinct=5, max_doc_freq=3, max_total_freq=18)
    with packed_env(MMT_GUIDED_BATCH=9000, MMT_GUIDED_SLICE=limit, MUMEMTO_EXPAND=1):
        plan, text = observe(docs, wp, kw, 0, 1, True)
        check("slices/mem/0of1", plan)
        assert plan[0][0] > 0
        assert text == O.run(docs, **kw).text()
