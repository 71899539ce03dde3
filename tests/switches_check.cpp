// Stand-alone check of mumemto_amd/csrc/switches.hpp (tests/test_switches_host.py compiles it with the host sanitizers and
// runs it as a child process with a prepared environment).
//
//   switches_check values      one switch of each kind, as the accessors give it: one line for the test to compare
//   switches_check once_live   a `once` switch keeps its first value after setenv inside the process, a `live` one follows
#include "switches.hpp"

#include <cstdio>
#include <cstring>

static_assert(sw::info[(int)sw::Id::MMT_GUIDED_NO_RANK].kind == sw::K_present, "the presence switches stay presence switches");
static_assert(sw::info[(int)sw::Id::MMT_BIG_CAP].when == sw::W_once && sw::info[(int)sw::Id::MMT_GIANT_RANGE].when == sw::W_once,
              "switches of the sorter's round loop are read once");
static_assert(sizeof(sw::info) / sizeof(sw::info[0]) == (size_t)sw::Id::count, "one row per name");

static int fail(const char* what) { std::fprintf(stderr, "switches_check: %s\n", what); return 1; }

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "values")) {
        const char* t = sw::text(sw::MUMEMTO_PRODUCER);
        std::printf("present=%d flag=%d flag_set=%d on_unless_zero=%d int=%d u64=%llu text=%s%s%s\n",
                    (int)sw::on(sw::MMT_GUIDED_NO_RANK), (int)sw::on(sw::MMT_GUIDED_STAGE), (int)sw::is_set(sw::MMT_GUIDED_STAGE),
                    (int)sw::on(sw::MMT_SORT_FUSED), sw::num(sw::MMT_GIANT_RANGE, 65536),
                    (unsigned long long)sw::num(sw::MMT_GUIDED_SLICE, 7), t ? "[" : "unset", t ? t : "", t ? "]" : "");
        return 0;
    }
    if (!std::strcmp(mode, "once_live")) {
        // the test starts this with MMT_SORT_FUSED=0, MMT_BIG_CAP=5, MUMEMTO_POOL=0 (once) and MMT_GUIDED_BATCH=3000 (live)
        if (sw::on(sw::MMT_SORT_FUSED) || sw::num(sw::MMT_BIG_CAP, 9) != 5 || sw::num(sw::MMT_GUIDED_BATCH, 9) != 3000 ||
            sw::on(sw::MMT_GUIDED_NO_RANK) || sw::is_set(sw::MUMEMTO_HEAP_LIMIT))
            return fail("first reads");
        const char* pool = sw::text(sw::MUMEMTO_POOL);
        if (!pool || std::strcmp(pool, "0")) return fail("first read of a once text");
        setenv("MMT_SORT_FUSED", "1", 1); setenv("MMT_BIG_CAP", "77", 1); setenv("MUMEMTO_POOL", "a longer value than before", 1);
        setenv("MUMEMTO_HEAP_LIMIT", "4096", 1);                 // (unset at the first read: stays unset)
        setenv("MMT_GUIDED_BATCH", "4000", 1); setenv("MMT_GUIDED_NO_RANK", "0", 1);
        if (sw::on(sw::MMT_SORT_FUSED) || sw::num(sw::MMT_BIG_CAP, 9) != 5 || sw::is_set(sw::MUMEMTO_HEAP_LIMIT) ||
            sw::num(sw::MUMEMTO_HEAP_LIMIT, 0) != 0)
            return fail("a once switch followed setenv");
        if (sw::text(sw::MUMEMTO_POOL) != pool || std::strcmp(pool, "0")) return fail("a once text followed setenv");
        if (sw::num(sw::MMT_GUIDED_BATCH, 9) != 4000 || !sw::on(sw::MMT_GUIDED_NO_RANK)) return fail("a live switch did not follow setenv");
        unsetenv("MMT_GUIDED_BATCH"); unsetenv("MMT_GUIDED_NO_RANK"); unsetenv("MMT_BIG_CAP");
        if (sw::is_set(sw::MMT_GUIDED_BATCH) || sw::on(sw::MMT_GUIDED_NO_RANK)) return fail("a live switch did not follow unsetenv");
        if (!sw::is_set(sw::MMT_BIG_CAP)) return fail("a once switch followed unsetenv");
        std::printf("once_live ok\n");
        return 0;
    }
    return fail("usage: switches_check values | once_live");
}
