// Every MMT_* / MUMEMTO_* environment variable the library and its tools read, through one typed table (switches.def).
// Header-only: extract_mums is built from fasta.cpp alone by a plain host compiler.
//
//   sw::on(sw::MMT_GUIDED_NO_RANK)        present / flag / on_unless_zero
//   sw::is_set(sw::MMT_GUIDED_STAGE)      any kind ("unset = automatic" of the tri-state flags)
//   sw::num(sw::MMT_GIANT_RANGE, 65536)   int (atoi) / u64 (strtoull, base 10); the default when unset
//   sw::text(sw::MUMEMTO_PRODUCER)        text: the raw string, nullptr when unset
//
// A name that is not in the table does not compile, and neither does an accessor that does not fit the entry's kind.
// A `once` entry is read at its first use and keeps that value for the life of the process; a `live` one is read from the
// environment at every call.  Defaults and clamps that belong to a call site stay at the call site.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>

namespace sw {

enum Kind { K_present, K_flag, K_on_unless_zero, K_int, K_u64, K_text };
enum When { W_once, W_live };

enum class Id : int {
#define MMT_SWITCH(name, kind, when, doc) name,
#include "switches.def"
#undef MMT_SWITCH
    count
};

struct Info { const char* name; Kind kind; When when; };
inline constexpr Info info[] = {
#define MMT_SWITCH(name, kind, when, doc) {#name, K_##kind, W_##when},
#include "switches.def"
#undef MMT_SWITCH
};

// one type per entry: the accessors check the kind at compile time and a `once` entry gets a cache of its own
template <Id I> struct Switch {
    static constexpr const char* name = info[(int)I].name;
    static constexpr Kind kind = info[(int)I].kind;
    static constexpr bool once = info[(int)I].when == W_once;
};
#define MMT_SWITCH(name, kind, when, doc) inline constexpr Switch<Id::name> name{};
#include "switches.def"
#undef MMT_SWITCH

// the value as the environment has it, nullptr when unset (a `once` entry: as it had it at the first call)
template <Id I> inline const char* raw(Switch<I>) {
    if constexpr (Switch<I>::once) {
        struct First { bool set; std::string value; };
        static const First first = [] { const char* e = std::getenv(Switch<I>::name); return First{e != nullptr, e ? e : ""}; }();
        return first.set ? first.value.c_str() : nullptr;
    } else {
        return std::getenv(Switch<I>::name);
    }
}

template <Id I> inline bool is_set(Switch<I> s) { return raw(s) != nullptr; }

template <Id I> inline bool on(Switch<I> s) {
    constexpr Kind k = Switch<I>::kind;
    static_assert(k == K_present || k == K_flag || k == K_on_unless_zero, "sw::on wants a present, flag or on_unless_zero switch");
    const char* e = raw(s);
    if constexpr (k == K_present) return e != nullptr;
    else if constexpr (k == K_flag) return e && std::atoi(e) != 0;
    else return !(e && std::atoi(e) == 0);
}

template <Id I> using Num = std::conditional_t<Switch<I>::kind == K_u64, uint64_t, int>;
template <Id I> inline Num<I> num(Switch<I> s, Num<I> dflt) {
    constexpr Kind k = Switch<I>::kind;
    static_assert(k == K_int || k == K_u64, "sw::num wants an int or u64 switch");
    const char* e = raw(s);
    if (!e) return dflt;
    if constexpr (k == K_int) return std::atoi(e);
    else return (uint64_t)std::strtoull(e, nullptr, 10);
}

template <Id I> inline const char* text(Switch<I> s) {
    static_assert(Switch<I>::kind == K_text, "sw::text wants a text switch");
    return raw(s);
}

}  // namespace sw
