"""DoublingSorter::sort as a unit, in the three forms it is called in (byte text, PFP dictionary with and without
RunRefine, integer parse), through the probe library against an independent prefix-doubling sort in numpy
(tests/kprobe.py, checked on the CPU by tests/test_sorter_reference_host.py).  Inputs on which prefix doubling needs
every round: one-letter, periodic, Fibonacci and Thue-Morse strings, letter runs, a huge alphabet with one frequent
symbol.  sa equals the reference, rank is its inverse, the rounds stay within ceil(log2(n / h0)) + 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kprobe as K
import sorter_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("n", (1, 2, 3, 4095, 4096, 4097, 20000))
def test_three_call_forms(n):
    out = C.form_cases((n,))
    assert len(out) == 8 * 4 + 1          # eight inputs in four forms (text, dictionary without and with RunRefine, integers) + the big alphabet


def test_run_refine_took_part():
    """RunRefine orders a run bucket below the default threshold only with MMT_RUN_BUCKET lowered (set around the one call
    and restored), and the variable does not leak into the tests that follow"""
    before = os.environ.get("MMT_RUN_BUCKET")
    text = K.text_inputs(4097)["a^n"]
    d, code, bits, chars, sigma = K.dict_form(text)
    assert bits <= 3
    want = K.ref_suffix_array(code[d], terminator=0)
    sa, rank, rounds, refined = K.sorter_text(d, code, bits, chars, sigma, sep_code=int(code[1]), use_runs=True)
    if before is None:
        assert refined == 0, "a bucket below 4096 suffixes was refined at the default threshold"
    assert np.array_equal(sa, want)
    with K.environment(MMT_RUN_BUCKET="2"):
        sa, rank, rounds, refined = K.sorter_text(d, code, bits, chars, sigma, sep_code=int(code[1]), use_runs=True)
    assert 0 < refined < 4096 and np.array_equal(sa, want)
    assert os.environ.get("MMT_RUN_BUCKET") == before


def _child(env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "sorter_cases.py"), "forms_digest"], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sorter cases ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return [l for l in r.stdout.splitlines() if l.startswith("sa digest")][0]


def test_switch_settings_agree():
    """the periodic and run inputs under the round of separate kernels, the small tile, a long-range list of one entry
    and device-wide rounds: one child per setting, each checked against the reference, all with the same suffix arrays"""
    here = "sa digest " + C.sa_digest(C.form_cases((4097, 20000), K.PERIODIC_AND_RUNS))
    for env in ({"MMT_SORT_FUSED": "0"}, {"MMT_ROUND_CAP": "1024"}, {"MMT_BIG_CAP": "1"}, {"MMT_SORT_GLOBAL_ROUNDS": "1"}):
        assert _child(env) == here, env


def test_probe_beside_the_library():
    """the probe carries its own device heap: it must work in a process that has libmumemto.so loaded and running"""
    import mumemto_amd
    from mumemto_amd import synth
    eng = mumemto_amd.Engine(0)
    eng.set_docs(synth.pangenome(3, 3000, 0.01, seed=2))
    eng.run()
    first = eng.output_text()
    assert K.scan(4, np.full(3, 0xC0000000, np.uint32), np.uint64).tolist() == [0, 0xC0000000, 0x180000000]
    out = C.form_cases((4097,), ("(ab)^n",))
    assert len(out) == 4
    eng.run()
    assert eng.output_text() == first
    eng.close()
