"""The environment switches (mumemto_amd/csrc/switches.def, read through switches.hpp): the table is the only reader, every
line of it is used, no test or document names a switch that does not exist, and the accessors give what the parsing idioms
they replaced gave.  Host only."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mumemto_amd", "csrc")
NAME = re.compile(r"\b(?:MMT|MUMEMTO)_[A-Z0-9_]+")
KINDS = {"present", "flag", "on_unless_zero", "int", "u64", "text"}

# names that only Python reads (each with its reader); everything else must be a line of switches.def
PYTHON_ONLY = {
    "MUMEMTO_NO_TORCH",             # mumemto_amd/binding.py: the ctypes binding without torch
    "MMT_FUZZ_CASES",               # tests/test_oracle_fuzz.py: seeded cases per mode
    "MMT_FUZZ_SHARDS",              # tests/fuzz_run.py: every case once more as shards of the scan
    "MMT_GPU_BRUTEFORCE_CASES",     # tests/test_gpu_bruteforce.py: number of cases
}
# tokens of that shape that are no environment variables
NOT_SWITCHES = {
    "MMT_SWITCH",                   # the X-macro of switches.def itself
    "MMT_API", "MUMEMTO_EXPORT",    # the export macros of include/ (tests/test_library_loads.py and others read the headers)
}


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def table():
    rows = re.findall(r'^MMT_SWITCH\((\w+),\s*(\w+),\s*(\w+),\s*"(.+)"\)$', read(os.path.join(CSRC, "switches.def")), re.M)
    assert len(rows) == len(re.findall(r"^MMT_SWITCH\(", read(os.path.join(CSRC, "switches.def")), re.M))
    return rows


def native_sources():
    files = [p for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".cpp", ".hpp", ".hip", ".h"))]
    return files + glob.glob(os.path.join(ROOT, "include", "*"))


def test_table_is_well_formed():
    rows = table()
    names = [r[0] for r in rows]
    assert len(names) == len(set(names)) == 100
    for name, kind, when, doc in rows:
        assert NAME.fullmatch(name), name
        assert kind in KINDS and when in ("once", "live"), name
        assert len(doc) > 20 and doc.endswith("."), name


def test_no_stray_reads():
    """Outside switches.hpp nothing reads a prefixed name from the environment; a getenv of a computed name could."""
    for path in native_sources():
        if os.path.basename(path) == "switches.hpp":
            continue
        for m in re.finditer(r"getenv\s*\(\s*([^)]*)\)", read(path)):
            arg = m.group(1).strip()
            assert re.fullmatch(r'"[^"]*"', arg) and not NAME.search(arg), (os.path.relpath(path, ROOT), m.group(0))


def test_every_entry_is_used():
    text = "\n".join(read(p) for p in native_sources() if os.path.basename(p) != "switches.hpp")
    unused = [name for name, _, _, _ in table() if not re.search(r"\bsw::%s\b" % name, text)]
    assert not unused, unused


def test_no_unknown_names_in_python_and_documents():
    """A misspelt name in a test's env= dict runs the default path and passes: every name the tests, the benchmark, the package
    and the two user documents mention is a line of the table (or on the two short lists above)."""
    known = {r[0] for r in table()} | PYTHON_ONLY | NOT_SWITCHES
    files = glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "mumemto_amd", "*.py"))
    files += [os.path.join(ROOT, f) for f in ("bench.py", "README.md", "INTEGRATION.md")]
    unknown = {}
    for path in files:
        for tok in NAME.findall(read(path)):
            # ("MMT_GUIDED_NO_*" and the like: a family of names, named by its prefix)
            if tok not in known and not (tok.endswith("_") and any(k.startswith(tok) for k in known)):
                unknown.setdefault(tok, set()).add(os.path.relpath(path, ROOT))
    assert not unknown, unknown


# ---- the accessors, by a stand-alone program under the host sanitizers ----

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("switches") / "switches_check")
    # (the sanitizers' runtimes inside the program: it runs as it is, whatever the environment preloads)
    subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "switches_check.cpp"), "-o", exe], check=True)
    return exe


def run_checker(exe, mode, env):
    base = {k: v for k, v in os.environ.items() if not NAME.fullmatch(k)}
    r = subprocess.run([exe, mode], env=dict(base, **env), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


# what the idioms the table replaced give:  present  `getenv(X) != nullptr`;  flag  `atoi(c) != 0` (and "is it set");
# on_unless_zero  `!(getenv(X) && atoi(getenv(X)) == 0)`;  int  `getenv(X) ? atoi(..) : 65536`;  u64  `getenv(X) ? strtoull(.., 10) : 7`
#            value     present flag set  on_unless_zero int    u64 text
VALUES = [(None,    0, 0, 0, 1, 65536, 7, "unset"),
          ("",      1, 0, 1, 0, 0, 0, "[]"),
          ("0",     1, 0, 1, 0, 0, 0, "[0]"),
          ("1",     1, 1, 1, 1, 1, 1, "[1]"),
          ("17",    1, 1, 1, 1, 17, 17, "[17]"),
          ("junk",  1, 0, 1, 0, 0, 0, "[junk]")]


@pytest.mark.parametrize("case", VALUES, ids=lambda c: repr(c[0]))
def test_values_of_each_kind(checker, case):
    value, present, flag, is_set, on_unless_zero, as_int, as_u64, text = case
    names = ("MMT_GUIDED_NO_RANK", "MMT_GUIDED_STAGE", "MMT_SORT_FUSED", "MMT_GIANT_RANGE", "MMT_GUIDED_SLICE", "MUMEMTO_PRODUCER")
    kinds = {r[0]: r[1] for r in table()}
    assert [kinds[n] for n in names] == ["present", "flag", "on_unless_zero", "int", "u64", "text"]
    env = {} if value is None else {n: value for n in names}
    assert run_checker(checker, "values", env) == "present=%d flag=%d flag_set=%d on_unless_zero=%d int=%d u64=%d text=%s" % (
        present, flag, is_set, on_unless_zero, as_int, as_u64, text)


def test_once_keeps_its_first_value_and_live_follows(checker):
    when = {r[0]: r[2] for r in table()}
    assert [when[n] for n in ("MMT_SORT_FUSED", "MMT_BIG_CAP", "MUMEMTO_POOL", "MUMEMTO_HEAP_LIMIT")] == ["once"] * 4
    assert [when[n] for n in ("MMT_GUIDED_BATCH", "MMT_GUIDED_NO_RANK")] == ["live"] * 2
    env = dict(MMT_SORT_FUSED="0", MMT_BIG_CAP="5", MUMEMTO_POOL="0", MMT_GUIDED_BATCH="3000")
    assert run_checker(checker, "once_live", env) == "once_live ok"


@pytest.mark.parametrize("line", ["sw::num(sw::MMT_GUIDED_NO_RANK, 0)",        # a number of a presence switch
                                  "sw::on(sw::MMT_GUIDED_BATCH)",             # on / off of a number
                                  "sw::text(sw::MMT_GUIDED_STAGE)",           # the string of a flag
                                  "sw::on(sw::MMT_GUIDED_NO_rank)"])          # a misspelt name
def test_wrong_kind_or_name_does_not_compile(tmp_path, line):
    src = tmp_path / "wrong.cpp"
    src.write_text('#include "switches.hpp"\nint main() { return (int)(bool)%s; }\n' % line)
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    ok = tmp_path / "right.cpp"
    ok.write_text('#include "switches.hpp"\nint main() { return (int)sw::on(sw::MMT_GUIDED_NO_RANK); }\n')
    assert subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", CSRC, str(ok)], capture_output=True).returncode == 0
    assert subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True).returncode != 0
