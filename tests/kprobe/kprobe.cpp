// kprobe.cpp -- test infrastructure: plain C entry points around single launch wrappers of the suffix sorter
// (mmt::k, mmt::prims, pk::pack_keys_u32, DoublingSorter::sort), of the prefix-free parse (mmt::pk rows A2-A4, the
// dictionary's LCP steps of mmt::k, build_rmq / ParseLcp::build / rmq_min of parse_lcp.hpp) and of the bucket-wise producer
// (mmt::gk, guided_kernels.hpp: the kp_gk_* functions at the end), for tests/kprobe.py.
//
// Every kp_* function takes host arrays, uploads them, calls exactly ONE wrapper, synchronises and copies the results
// back; arrays marked "in/out" go up as the caller filled them (sentinel patterns: what the wrapper must not touch
// comes back unchanged).  Errors: a non-zero return code, the message through kp_last_error() (as mmt_last_error).
// The library links the product's own objects (the classes are hidden symbols of libmumemto.so), so it carries its
// own copy of the device heap and of the switch table; nothing of the product is restated here.
//
// Adding a wrapper: one KP function below (upload with Dev<T>, call, down()), one ctypes line in tests/kprobe.py.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "device_utils.hpp"
#include "guided_kernels.hpp"
#include "kernels.hpp"
#include "parse_lcp.hpp"
#include "pfp_kernels.hpp"
#include "prims.hpp"
#include "sorter.hpp"

using namespace mmt;

#define KP extern "C" __attribute__((visibility("default")))

static std::string g_err;
static hipStream_t g_stream = nullptr;

static hipStream_t stream() {
    if (!g_stream) MMT_HIP(hipStreamCreate(&g_stream));
    return g_stream;
}
static void sync() { MMT_HIP(hipStreamSynchronize(stream())); }

template <typename F>
static int guarded(F&& f) {
    try { f(); sync(); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return 1; }
    catch (...) { g_err = "unknown error"; return 2; }
}

// a host array on the device (at least one element is allocated: a null host pointer uploads nothing)
template <typename T>
struct Dev {
    DevBuf<T> b;
    size_t n;
    Dev(const T* h, size_t n_) : n(n_) {
        b.ensure(n ? n : 1);
        if (n && h) { MMT_HIP(hipMemcpyAsync(b.get(), h, n * sizeof(T), hipMemcpyHostToDevice, stream())); sync(); }
    }
    T* p() { return b.get(); }
    void down(T* h) {
        sync();
        if (n && h) { MMT_HIP(hipMemcpyAsync(h, b.get(), n * sizeof(T), hipMemcpyDeviceToHost, stream())); sync(); }
    }
};
typedef uint32_t u32;
typedef uint64_t u64;
typedef uint8_t u8;

KP const char* kp_last_error() { return g_err.c_str(); }
KP u32 kp_round_fused_cap() { return k::round_fused_cap(); }
KP u32 kp_round_tile_cap() { return k::ROUND_TILE_CAP; }

// ---- first keys --------------------------------------------------------------------------------------------------
// run_ends: in/out, run_alloc entries (run_cap <= run_alloc of them may be written); run_count: in/out, one entry
KP int kp_pack_keys(const u8* text, u32 n, const u8* code, int bits, int chars, u32 sep_code, u64* keys, u32* vals,
                    u32* run_ends, u32 run_alloc, u32* run_count, u32 run_cap) {
    return guarded([&] {
        Dev<u8> t(text, n), c(code, 256);
        Dev<u64> dk(nullptr, n);
        Dev<u32> dv(nullptr, n), re(run_ends, run_alloc), rc(run_count, 1);
        k::pack_keys(t.p(), n, c.p(), bits, chars, sep_code, dk.p(), dv.p(), stream(), run_ends ? re.p() : nullptr,
                     run_ends ? rc.p() : nullptr, run_cap);
        dk.down(keys); dv.down(vals); re.down(run_ends); rc.down(run_count);
    });
}
KP int kp_pack_keys_u32(const u32* parse, u32 m, int bits, int chars, u64* keys, u32* vals) {
    return guarded([&] {
        Dev<u32> p(parse, m), dv(nullptr, m);
        Dev<u64> dk(nullptr, m);
        pk::pack_keys_u32(p.p(), m, bits, chars, dk.p(), dv.p(), stream());
        dk.down(keys); dv.down(vals);
    });
}
KP int kp_equal_range_u64(const u64* sorted, u32 n, const u64* probe, u32 n_probes, u32* lo_hi) {
    return guarded([&] {
        Dev<u64> a(sorted, n), p(probe, n_probes);
        Dev<u32> o(nullptr, 2 * (size_t)n_probes);
        k::equal_range_u64(a.p(), n, p.p(), n_probes, o.p(), stream());
        o.down(lo_hi);
    });
}
KP int kp_run_keys(const u32* sa, u32 cnt, const u8* text, u32 n, const u8* code, int bits, int chars, const u32* ends,
                   u32 n_ends, u64* key2) {
    return guarded([&] {
        Dev<u32> a(sa, cnt), e(ends, n_ends);
        Dev<u8> t(text, n), c(code, 256);
        Dev<u64> o(nullptr, cnt);
        k::run_keys(a.p(), cnt, t.p(), n, c.p(), bits, chars, e.p(), n_ends, o.p(), stream());
        o.down(key2);
    });
}

// ---- heads and ranks ---------------------------------------------------------------------------------------------
KP int kp_mark_heads(const u64* keys, u32 n, int lsb_unique, u32* headval) {
    return guarded([&] {
        Dev<u64> a(keys, n);
        Dev<u32> o(nullptr, n);
        k::mark_heads(a.p(), n, o.p(), lsb_unique != 0, stream());
        o.down(headval);
    });
}
KP int kp_force_heads(u32* headval, u32 n, const u32* at, u32 cnt) {          // headval: in/out
    return guarded([&] {
        Dev<u32> h(headval, n), a(at, cnt);
        k::force_heads(h.p(), a.p(), cnt, n, stream());
        h.down(headval);
    });
}
KP int kp_scatter_rank(const u32* sa, const u32* head, u32 n, u32* rank, u32 rank_len) {      // rank: in/out
    return guarded([&] {
        Dev<u32> a(sa, n), h(head, n), r(rank, rank_len);
        k::scatter_rank(a.p(), h.p(), n, r.p(), stream());
        r.down(rank);
    });
}
KP int kp_scatter_rank_changed(const u32* sa, const u32* head, const u32* old_head, u32 m, u32* rank, u32 rank_len) {
    return guarded([&] {
        Dev<u32> a(sa, m), h(head, m), o(old_head, m), r(rank, rank_len);
        k::scatter_rank_changed(a.p(), h.p(), o.p(), m, r.p(), stream());
        r.down(rank);
    });
}
KP int kp_flag_unsorted(const u32* head, u32 n, u8* flags) {
    return guarded([&] {
        Dev<u32> h(head, n);
        Dev<u8> f(nullptr, n);
        k::flag_unsorted(h.p(), n, f.p(), stream());
        f.down(flags);
    });
}
// out: in/out, n entries; count: in/out
KP int kp_select_indices(const u8* flags, u32 n, u32* out, u32* count) {
    return guarded([&] {
        Dev<u8> f(flags, n), temp(nullptr, 0);
        Dev<u32> o(out, n), c(count, 1);
        prims::select_indices(temp.b, f.p(), o.p(), c.p(), n, stream());
        o.down(out); c.down(count);
    });
}
KP int kp_select_tied_heads(const u32* head, u32 n, u32* out, u32* count) {
    return guarded([&] {
        Dev<u8> temp(nullptr, 0);
        Dev<u32> h(head, n), o(out, n), c(count, 1);
        prims::select_tied_heads(temp.b, h.p(), o.p(), c.p(), n, stream());
        o.down(out); c.down(count);
    });
}
KP int kp_gather_active(const u32* idx, u32 m, const u32* sa, const u32* head, u32 n, u32* out_pos, u32* out_sa,
                        u32* out_head) {
    return guarded([&] {
        Dev<u32> i(idx, m), a(sa, n), h(head, n), op(nullptr, m), os(nullptr, m), oh(nullptr, m);
        k::gather_active(i.p(), m, a.p(), h.p(), op.p(), os.p(), oh.p(), stream());
        op.down(out_pos); os.down(out_sa); oh.down(out_head);
    });
}
KP int kp_compact_round(const u32* idx, u32 m2, const u32* pos, const u32* sa_sorted, const u32* newhead, u32 m,
                        u32* out_pos, u32* out_sa, u32* out_head) {
    return guarded([&] {
        Dev<u32> i(idx, m2), p(pos, m), a(sa_sorted, m), h(newhead, m), op(nullptr, m2), os(nullptr, m2), oh(nullptr, m2);
        k::compact_round(i.p(), m2, p.p(), a.p(), h.p(), op.p(), os.p(), oh.p(), stream());
        op.down(out_pos); os.down(out_sa); oh.down(out_head);
    });
}
KP int kp_mark_subheads(const u64* keys, const u32* pos, u32 m, u32* headval) {
    return guarded([&] {
        Dev<u64> a(keys, m);
        Dev<u32> p(pos, m), o(nullptr, m);
        k::mark_subheads(a.p(), p.p(), m, o.p(), stream());
        o.down(headval);
    });
}
// sa (n entries), rank (n entries): in/out
KP int kp_apply_round(const u32* sa_sorted, const u32* newhead, const u32* pos, u32 m, u32* sa, u32* rank, u32 n,
                      u8* flags) {
    return guarded([&] {
        Dev<u32> a(sa_sorted, m), h(newhead, m), p(pos, m), dsa(sa, n), dr(rank, n);
        Dev<u8> f(nullptr, m);
        k::apply_round(a.p(), h.p(), p.p(), m, dsa.p(), dr.p(), f.p(), stream());
        dsa.down(sa); dr.down(rank); f.down(flags);
    });
}

// ---- one doubling round ------------------------------------------------------------------------------------------
// rank: rank_len entries (the kernels read rank[i] for i < n only: n <= rank_len is the caller's business)
KP int kp_make_round_keys(const u32* sa_c, const u32* head_c, u32 m, const u32* rank, u32 rank_len, u32 n, u32 h,
                          int shift, u64* keys) {
    return guarded([&] {
        if (n > rank_len) throw std::runtime_error("kp_make_round_keys: n beyond the rank column");
        Dev<u32> a(sa_c, m), hd(head_c, m), r(rank, rank_len);
        Dev<u64> o(nullptr, m);
        k::make_round_keys(a.p(), hd.p(), m, r.p(), n, h, shift, o.p(), stream());
        o.down(keys);
    });
}
KP int kp_round_tile_bounds(const u64* keys, u32 m, int shift, u32 target, u32 limit, u32 n_tiles, u32* bound) {
    return guarded([&] {
        Dev<u64> a(keys, m);
        Dev<u32> b(nullptr, (size_t)n_tiles + 1);
        k::round_tile_bounds(a.p(), m, shift, target, limit, n_tiles, b.p(), stream());
        b.down(bound);
    });
}
KP int kp_round_head_bounds(const u32* headc, u32 m, u32 target, u32 limit, u32 n_tiles, u32* bound) {
    return guarded([&] {
        Dev<u32> a(headc, m), b(nullptr, (size_t)n_tiles + 1);
        k::round_head_bounds(a.p(), m, target, limit, n_tiles, b.p(), stream());
        b.down(bound);
    });
}
// kout, vout (m entries), big_begin, big_end (big_alloc >= big_cap entries), big_count: in/out
KP int kp_round_local_sort(const u64* kin, const u32* vin, u32 m, const u32* bound, u32 n_tiles, u64* kout, u32* vout,
                           u32* big_begin, u32* big_end, u32 big_alloc, u32* big_count, u32 big_cap, int shift) {
    return guarded([&] {
        if (big_cap > big_alloc) throw std::runtime_error("kp_round_local_sort: big_cap beyond the list");
        Dev<u64> a(kin, m), ko(kout, m);
        Dev<u32> v(vin, m), vo(vout, m), b(bound, (size_t)n_tiles + 1), bb(big_begin, big_alloc), be(big_end, big_alloc),
            bc(big_count, 1);
        k::round_local_sort(a.p(), v.p(), ko.p(), vo.p(), b.p(), n_tiles, bb.p(), be.p(), bc.p(), big_cap, shift, stream());
        ko.down(kout); vo.down(vout); bb.down(big_begin); be.down(big_end); bc.down(big_count);
    });
}
// sa (n entries), sac_out, head_out, flags (m entries), big_begin, big_end (big_alloc entries), big_count,
// tile_big (n_tiles + 1 entries): in/out
KP int kp_round_fused(const u32* sac, const u32* headc, const u32* pos, u32 m, const u32* bound, u32 n_tiles,
                      const u32* rank, u32 n, u32 h, int shift, u32* sa, u32* sac_out, u32* head_out, u8* flags,
                      u32* big_begin, u32* big_end, u32 big_alloc, u32* big_count, u32 big_cap, u8* tile_big) {
    return guarded([&] {
        if (big_cap > big_alloc) throw std::runtime_error("kp_round_fused: big_cap beyond the list");
        Dev<u32> a(sac, m), hd(headc, m), p(pos, m), b(bound, (size_t)n_tiles + 1), r(rank, n), dsa(sa, n), so(sac_out, m),
            ho(head_out, m), bb(big_begin, big_alloc), be(big_end, big_alloc), bc(big_count, 1);
        Dev<u8> f(flags, m), tb(tile_big, (size_t)n_tiles + 1);
        k::round_fused(a.p(), hd.p(), p.p(), b.p(), n_tiles, r.p(), n, h, shift, dsa.p(), so.p(), ho.p(), f.p(), bb.p(),
                       be.p(), bc.p(), big_cap, tb.p(), stream());
        dsa.down(sa); so.down(sac_out); ho.down(head_out); f.down(flags); bb.down(big_begin); be.down(big_end);
        bc.down(big_count); tb.down(tile_big);
    });
}
// keys (m entries): in/out
KP int kp_round_big_keys(const u8* tile_big, const u32* bound, u32 target, u32 n_tiles, const u32* sac, const u32* headc,
                         u32 m, const u32* rank, u32 rank_len, u32 n, u32 h, int shift, u64* keys) {
    return guarded([&] {
        if (n > rank_len) throw std::runtime_error("kp_round_big_keys: n beyond the rank column");
        Dev<u8> tb(tile_big, (size_t)n_tiles + 1);
        Dev<u32> b(bound, (size_t)n_tiles + 1), a(sac, m), hd(headc, m), r(rank, rank_len);
        Dev<u64> o(keys, m);
        k::round_big_keys(tb.p(), b.p(), target, n_tiles, a.p(), hd.p(), r.p(), n, h, shift, o.p(), stream());
        o.down(keys);
    });
}
// head (m entries): in/out
KP int kp_round_big_subheads(const u8* tile_big, const u32* bound, u32 target, u32 n_tiles, const u64* keys,
                             const u32* pos, u32 m, u32* head) {
    return guarded([&] {
        Dev<u8> tb(tile_big, (size_t)n_tiles + 1);
        Dev<u32> b(bound, (size_t)n_tiles + 1), p(pos, m), o(head, m);
        Dev<u64> a(keys, m);
        k::round_big_subheads(tb.p(), b.p(), target, n_tiles, a.p(), p.p(), o.p(), stream());
        o.down(head);
    });
}
// sa (n entries), flags (m entries): in/out
KP int kp_round_big_apply(const u8* tile_big, const u32* bound, u32 target, u32 n_tiles, u32 m, const u32* sa_sorted,
                          const u32* head, const u32* pos, u32* sa, u32 n, u8* flags) {
    return guarded([&] {
        Dev<u8> tb(tile_big, (size_t)n_tiles + 1), f(flags, m);
        Dev<u32> b(bound, (size_t)n_tiles + 1), a(sa_sorted, m), hd(head, m), p(pos, m), dsa(sa, n);
        k::round_big_apply(tb.p(), b.p(), target, n_tiles, m, a.p(), hd.p(), p.p(), dsa.p(), f.p(), stream());
        dsa.down(sa); f.down(flags);
    });
}

// ---- prims -------------------------------------------------------------------------------------------------------
KP int kp_sort_pairs_u64_u32(const u64* kin, const u32* vin, u32 n, int begin_bit, int end_bit, u64* kout, u32* vout) {
    return guarded([&] {
        Dev<u8> temp(nullptr, 0);
        Dev<u64> a(kin, n), ko(nullptr, n);
        Dev<u32> v(vin, n), vo(nullptr, n);
        prims::sort_pairs_u64_u32(temp.b, a.p(), ko.p(), v.p(), vo.p(), n, begin_bit, end_bit, stream());
        ko.down(kout); vo.down(vout);
    });
}
// the four range sorts: key_bytes / val_bytes 4 or 8; kout, vout (n entries): in/out
template <typename K, typename V>
static void ranges_typed(const void* kin, const void* vin, void* kout, void* vout, u32 n, u32 segments, const u32* begin,
                         const u32* end, int end_bit, bool ordered) {
    Dev<u8> temp(nullptr, 0);
    Dev<K> a((const K*)kin, n), ko((const K*)kout, n);
    Dev<V> v((const V*)vin, n), vo((const V*)vout, n);
    Dev<u32> b(begin, segments), e(end, segments);
    if constexpr (sizeof(K) == 4 && sizeof(V) == 4)
        prims::segmented_sort_pairs_u32_ranges(temp.b, a.p(), ko.p(), v.p(), vo.p(), n, segments, b.p(), e.p(), end_bit, stream());
    else if constexpr (sizeof(K) == 4)
        prims::segmented_sort_pairs_u32_u64vals_ranges(temp.b, a.p(), ko.p(), v.p(), vo.p(), n, segments, b.p(), e.p(), end_bit, stream());
    else if constexpr (sizeof(V) == 4)
        prims::segmented_sort_pairs_u64_ranges(temp.b, a.p(), ko.p(), v.p(), vo.p(), n, segments, b.p(), e.p(), end_bit, stream(), ordered);
    else
        prims::segmented_sort_pairs_u64_u64vals_ranges(temp.b, a.p(), ko.p(), v.p(), vo.p(), n, segments, b.p(), e.p(), end_bit, stream());
    ko.down((K*)kout); vo.down((V*)vout);
}
KP int kp_sort_ranges(int key_bytes, int val_bytes, const void* kin, const void* vin, void* kout, void* vout, u32 n,
                      u32 segments, const u32* begin, const u32* end, int end_bit, int keys_order_the_ranges) {
    return guarded([&] {
        const bool o = keys_order_the_ranges != 0;
        if (o && !(key_bytes == 8 && val_bytes == 4)) throw std::runtime_error("kp_sort_ranges: keys_order_the_ranges is a switch of the u64 / u32 form");
        if (key_bytes == 4 && val_bytes == 4) ranges_typed<u32, u32>(kin, vin, kout, vout, n, segments, begin, end, end_bit, o);
        else if (key_bytes == 4 && val_bytes == 8) ranges_typed<u32, u64>(kin, vin, kout, vout, n, segments, begin, end, end_bit, o);
        else if (key_bytes == 8 && val_bytes == 4) ranges_typed<u64, u32>(kin, vin, kout, vout, n, segments, begin, end, end_bit, o);
        else if (key_bytes == 8 && val_bytes == 8) ranges_typed<u64, u64>(kin, vin, kout, vout, n, segments, begin, end, end_bit, o);
        else throw std::runtime_error("kp_sort_ranges: key / value width");
    });
}
// the scans: 0 inclusive_max_u32 (in place), 1 inclusive_segmin_u64 (in place), 2 exclusive_sum_u32, 3 inclusive_sum_u32,
// 4 exclusive_sum_u32_to_u64, 5 exclusive_sum_u64; `in` and `out` hold n entries of the widths that form has
KP int kp_scan(int which, const void* in, void* out, u32 n) {
    return guarded([&] {
        Dev<u8> temp(nullptr, 0);
        if (which == 0) { Dev<u32> a((const u32*)in, n); prims::inclusive_max_u32(temp.b, a.p(), a.p(), n, stream()); a.down((u32*)out); }
        else if (which == 1) { Dev<u64> a((const u64*)in, n); prims::inclusive_segmin_u64(temp.b, a.p(), a.p(), n, stream()); a.down((u64*)out); }
        else if (which == 2) { Dev<u32> a((const u32*)in, n), o(nullptr, n); prims::exclusive_sum_u32(temp.b, a.p(), o.p(), n, stream()); o.down((u32*)out); }
        else if (which == 3) { Dev<u32> a((const u32*)in, n), o(nullptr, n); prims::inclusive_sum_u32(temp.b, a.p(), o.p(), n, stream()); o.down((u32*)out); }
        else if (which == 4) { Dev<u32> a((const u32*)in, n); Dev<u64> o(nullptr, n); prims::exclusive_sum_u32_to_u64(temp.b, a.p(), o.p(), n, stream()); o.down((u64*)out); }
        else if (which == 5) { Dev<u64> a((const u64*)in, n), o(nullptr, n); prims::exclusive_sum_u64(temp.b, a.p(), o.p(), n, stream()); o.down((u64*)out); }
        else throw std::runtime_error("kp_scan: which");
    });
}

// ---- the sorter in its call forms ----------------------------------------------------------------------------------
// Byte text (sep_code = PACK_NO_SEP, key_bits = bits * chars: the engine) or dictionary (sep_code a symbol code,
// key_bits = bits * chars + 1, lsb_unique; use_runs: the ends of the long runs listed by pack_keys, sorted and handed
// over as RunRefine, as the parse stage does).  out[0] = rounds, out[1] = run_refined().
KP int kp_sorter_text(const u8* text, u32 n, const u8* code, int bits, int chars, int sigma, u32 sep_code, int use_runs,
                      u32* sa, u32* rank, u64* out) {
    return guarded([&] {
        const bool dict = sep_code != k::PACK_NO_SEP;
        Dev<u8> t(text, n), c(code, 256), temp(nullptr, 0);
        Dev<u32> dsa(nullptr, n), dr(nullptr, n);
        const u32 run_cap = 1u << 16;
        Dev<u32> ends(nullptr, use_runs ? run_cap : 0), cnt(nullptr, 1);
        DevBuf<u32> sorted;
        MMT_HIP(hipMemsetAsync(cnt.p(), 0, 4, stream()));
        DoublingSorter S;
        S.reserve(n);
        k::pack_keys(t.p(), n, c.p(), bits, chars, sep_code, S.keys_in(), S.vals_in(), stream(), use_runs ? ends.p() : nullptr,
                     use_runs ? cnt.p() : nullptr, run_cap);
        RunRefine runs;
        if (use_runs) {
            u32 found = 0;
            cnt.down(&found);
            if (found && found <= run_cap) {
                sorted.ensure((size_t)found * 3);
                MMT_HIP(hipMemsetAsync(sorted.get() + found, 0, (size_t)found * 4, stream()));
                prims::sort_pairs_u32_u32(temp.b, ends.p(), sorted.get(), sorted.get() + found, sorted.get() + 2 * (size_t)found,
                                          found, 0, 32, stream());
                runs.text = t.p(); runs.n = n; runs.code = c.p(); runs.bits = bits; runs.chars = chars; runs.sigma = sigma;
                runs.ends = sorted.get(); runs.n_ends = found;
            }
        }
        out[0] = (u64)S.sort(n, bits * chars + (dict ? 1 : 0), (u64)chars, dsa.p(), dr.p(), temp.b, stream(), dict,
                             runs.n_ends ? &runs : nullptr);
        out[1] = S.run_refined();
        dsa.down(sa); dr.down(rank);
    });
}
// the integer form (the parse): symbols of `bits` bits, `chars` of them per key
KP int kp_sorter_ints(const u32* parse, u32 m, int bits, int chars, u32* sa, u32* rank, u64* out) {
    return guarded([&] {
        Dev<u8> temp(nullptr, 0);
        Dev<u32> p(parse, m), dsa(nullptr, m), dr(nullptr, m);
        DoublingSorter S;
        S.reserve(m);
        pk::pack_keys_u32(p.p(), m, bits, chars, S.keys_in(), S.vals_in(), stream());
        out[0] = (u64)S.sort(m, bits * chars, (u64)chars, dsa.p(), dr.p(), temp.b, stream());
        out[1] = S.run_refined();
        dsa.down(sa); dr.down(rank);
    });
}

// ==== the prefix-free parse (pfp_kernels.hpp rows A2-A4, the dictionary's LCP steps of kernels.hpp, parse_lcp.hpp) =============
// Position tables go as untyped host pointers with `wide` (uint32_t or uint64_t entries), as the wrappers take them.  Before
// a launch every index a kernel will follow is checked on the host against the sizes the caller gave: a forged input that
// breaks a wrapper's precondition is an error message, never a stray access on the device.
static void need(bool ok, const char* what) { if (!ok) throw std::runtime_error(std::string("kprobe precondition: ") + what); }
static u64 pos_at(const void* a, bool wide, size_t i) { return wide ? ((const u64*)a)[i] : (u64)((const u32*)a)[i]; }
struct DevPos {                         // a position table (count entries of 4 or 8 bytes)
    Dev<u8> d; bool wide; size_t count;
    DevPos(const void* h, size_t n, bool w) : d((const u8*)h, n * (w ? 8 : 4)), wide(w), count(n) {}
    void* p() { return d.p(); }
    void down(void* h) { d.down((u8*)h); }
};

// The text as tests/kprobe.py hands it over.  BYTES (v != null): V = Dollar . T . Dollar^32 . zeros, v_len bytes of which at
// least 64 are zero padding; it is placed so that (v + 1) mod 16 = misalign (0: as Engine::text_ptr places it).  PACKED: the
// arrays of textref.hpp as the packer of tests/kprobe.py laid them out, uploaded as given.
struct KpText {
    const u8* v; u64 v_len; u32 misalign;
    const u64* packed; u64 n_words; const u64* excw; u64 n_excw; const ExcRun* runs; u32 n_runs;
    u64 n;
};
struct DevText {
    DevBuf<u8> bytes;
    Dev<u64> pk, ex;
    Dev<ExcRun> rn;
    TextRef T;
    u64 readable;                       // V indices below this may be read (bytes: v_len; packed: any -- tx_byte gives zeros)
    explicit DevText(const KpText* t)
        : pk(t->v ? nullptr : t->packed, t->v ? 0 : t->n_words), ex(t->v ? nullptr : t->excw, t->v ? 0 : t->n_excw),
          rn(t->v ? nullptr : t->runs, t->v ? 0 : t->n_runs) {
        T.n = t->n;
        if (t->v) {
            need(t->misalign < 16, "misalign 0..15");
            need(t->v_len >= t->n + 33 + 64, "V is Dollar, the text, 32 Dollars and at least 64 zero bytes");
            const size_t total = (size_t)t->v_len + 32 + 128;
            bytes.ensure(total);
            MMT_HIP(hipMemsetAsync(bytes.get(), 0, total, stream()));
            const uintptr_t base = reinterpret_cast<uintptr_t>(bytes.get());
            const size_t k = 16 + ((t->misalign + 32 - 1 - (base & 15)) & 15);          // (base + k + 1) mod 16 = misalign
            MMT_HIP(hipMemcpyAsync(bytes.get() + k, t->v, t->v_len, hipMemcpyHostToDevice, stream()));
            sync();
            T.v = bytes.get() + k;
            readable = t->v_len;
        } else {
            need(t->n_words >= (t->n + 31) / 32 + 2, "packed text: two words of padding");
            need(t->n_excw >= ((t->n >> TX_BLOCK_SHIFT) >> 6) + 1, "packed text: one flag per 4096 positions");
            T.packed = pk.p(); T.excw = ex.p(); T.runs = rn.p(); T.n_runs = t->n_runs;
            readable = ~0ull;
        }
    }
};

// ---- A2: triggers, cuts, phrases -----------------------------------------------------------------------------------
KP int kp_trigger_blocks(u64 n, u32* out) { return guarded([&] { *out = pk::trigger_blocks(n); }); }
KP int kp_emit_tile(u32* out) { return guarded([&] { *out = pk::emit_tile(); }); }
// masks (masks_len entries), block_count (count_len entries): in/out
KP int kp_trigger_masks(const KpText* tx, u64 n, u32 w, u32 p, uint16_t* masks, u32 masks_len, u32* block_count, u32 count_len) {
    return guarded([&] {
        need(n >= 1 && n == tx->n && w >= 1 && w <= 32 && p >= 1, "n = text length >= 1, 1 <= w <= 32, p >= 1");
        need(masks_len >= (n + 15) / 16 && count_len >= pk::trigger_blocks(n), "masks / block_count too short");
        DevText t(tx);
        Dev<uint16_t> m(masks, masks_len);
        Dev<u32> c(block_count, count_len);
        pk::trigger_masks(t.T, n, w, p, m.p(), c.p(), stream());
        m.down(masks); c.down(block_count);
    });
}
// cuts (cuts_len entries of 4 / 8 bytes): in/out
KP int kp_trigger_cuts(const uint16_t* masks, u64 n, const u32* block_off, void* cuts, u32 cuts_len, int wide) {
    return guarded([&] {
        const u64 threads = (n + 15) / 16;
        const u32 blocks = pk::trigger_blocks(n);
        for (u32 b = 0; b < blocks; b++) {
            u64 c = 0;
            for (u64 t = (u64)b * 256; t < std::min<u64>(threads, (u64)(b + 1) * 256); t++) c += __builtin_popcount(masks[t]);
            need((u64)block_off[b] + c <= cuts_len, "block_off + the block's triggers beyond the cut list");
        }
        Dev<uint16_t> m(masks, threads);
        Dev<u32> o(block_off, blocks);
        DevPos c(cuts, cuts_len, wide != 0);
        pk::trigger_cuts(m.p(), n, o.p(), c.p(), wide != 0, stream());
        c.down(cuts);
    });
}
// start, len (alloc entries): in/out
KP int kp_phrase_bounds(const void* cuts, u32 n_cuts, u64 n, u32 w, void* start, u32* len, u32 alloc, int wide) {
    return guarded([&] {
        need(alloc >= (u64)n_cuts + 1, "start / len hold n_cuts + 1 entries");
        DevPos c(cuts, n_cuts, wide != 0), s(start, alloc, wide != 0);
        Dev<u32> l(len, alloc);
        pk::phrase_bounds(c.p(), n_cuts, n, w, s.p(), l.p(), wide != 0, stream());
        s.down(start); l.down(len);
    });
}

// ---- A2: fingerprints and distinct phrases ---------------------------------------------------------------------------
// h1 (alloc entries), pinfo (4 * alloc words): in/out
KP int kp_phrase_hash(const KpText* tx, const void* start, const u32* len, u32 m, u64* h1, u32* pinfo, u32 alloc, int wide) {
    return guarded([&] {
        need(alloc >= m, "h1 / pinfo hold m entries");
        DevText t(tx);
        for (u32 k = 0; k < m; k++) need(pos_at(start, wide != 0, k) + len[k] <= t.readable, "a phrase beyond V");
        DevPos s(start, m, wide != 0);
        Dev<u32> l(len, m), pi(pinfo, 4 * (size_t)alloc);
        Dev<u64> h(h1, alloc);
        pk::phrase_hash(t.T, s.p(), l.p(), m, h.p(), pi.p(), wide != 0, stream());
        h.down(h1); pi.down(pinfo);
    });
}
KP int kp_second_fingerprint(const u32* pinfo, u32 m, u64* h2, u32 alloc) {                    // h2: in/out
    return guarded([&] {
        need(alloc >= m, "h2 holds m entries");
        Dev<u32> pi(pinfo, 4 * (size_t)m);
        Dev<u64> h(h2, alloc);
        pk::second_fingerprint(pi.p(), m, h.p(), stream());
        h.down(h2);
    });
}
// pinfo: n_rec records; flags (alloc entries), err (16 words): in/out
KP int kp_mark_distinct(const u32* order, const u64* h1s, const u32* pinfo, u32 n_rec, const KpText* tx, u32 m, u32* flags,
                        u32 alloc, u32* err) {
    return guarded([&] {
        need(alloc >= m, "flags holds m entries");
        DevText t(tx);
        for (u32 k = 0; k < m; k++) {
            need(order[k] < n_rec, "order beyond the records");
            const u32* r = pinfo + 4 * (size_t)order[k];
            need((((u64)(r[1] >> 24) << 32) | r[2]) + r[3] <= t.readable, "a record's phrase beyond V");
        }
        Dev<u32> o(order, m), pi(pinfo, 4 * (size_t)n_rec), f(flags, alloc), e(err, 16);
        Dev<u64> h(h1s, m);
        pk::mark_distinct(o.p(), h.p(), pi.p(), t.T, m, f.p(), e.p(), stream());
        f.down(flags); e.down(err);
    });
}
// pid (m entries), rep, dlen (d_alloc entries): in/out
KP int kp_assign_distinct(const u32* order, const u32* scan, const u32* flags, const u32* len, u32 m, u32* pid, u32* rep,
                          u32* dlen, u32 d_alloc) {
    return guarded([&] {
        for (u32 k = 0; k < m; k++) need(order[k] < m && scan[k] >= 1 && scan[k] <= d_alloc, "order / scan out of range");
        Dev<u32> o(order, m), sc(scan, m), f(flags, m), l(len, m), p(pid, m), r(rep, d_alloc), d(dlen, d_alloc);
        pk::assign_distinct(o.p(), sc.p(), f.p(), l.p(), m, p.p(), r.p(), d.p(), stream());
        p.down(pid); r.down(rep); d.down(dlen);
    });
}
KP int kp_sum_u32(const u32* x, u32 n, u64* out) {                                           // out: in/out, one entry
    return guarded([&] {
        Dev<u32> a(x, n);
        Dev<u64> o(out, 1);
        pk::sum_u32(a.p(), n, o.p(), stream());
        o.down(out);
    });
}

// ---- A2/A3: dictionary ------------------------------------------------------------------------------------------------
// start, len: n_phrases entries; dict (dict_alloc bytes), dinfo (dict_alloc entries, or null): in/out
KP int kp_copy_dict(const KpText* tx, const void* start, const u32* len, u32 n_phrases, const u32* which, const u32* dstart,
                    u32 n_phr, u8* dict, u64* dinfo, u32 dict_alloc, u32 dict_len, int pack_prev, int wide) {
    return guarded([&] {
        need(dict_len >= 1 && dict_len <= dict_alloc, "dict_len within the dictionary");
        DevText t(tx);
        for (u32 k = 0; k < n_phr; k++) {
            need(which[k] < n_phrases, "which beyond the phrases");
            need(len[which[k]] >= 1 && pos_at(start, wide != 0, which[k]) + len[which[k]] <= t.readable, "a phrase beyond V");
        }
        DevPos s(start, n_phrases, wide != 0);
        Dev<u32> l(len, n_phrases), wh(which, n_phr), ds(dstart, n_phr);
        Dev<u8> d(dict, dict_alloc);
        Dev<u64> di(dinfo, dinfo ? dict_alloc : 0);
        pk::copy_dict(t.T, s.p(), l.p(), wh.p(), ds.p(), n_phr, d.p(), dinfo ? di.p() : nullptr, dict_len, pack_prev != 0,
                      wide != 0, stream());
        d.down(dict); di.down(dinfo);
    });
}
// a dictionary on the device: nd bytes and the 64 zero bytes the product keeps behind them
struct DevDict {
    DevBuf<u8> b;
    DevDict(const u8* h, u32 nd) {
        b.ensure((size_t)nd + 128);
        MMT_HIP(hipMemsetAsync(b.get(), 0, (size_t)nd + 128, stream()));
        if (nd) MMT_HIP(hipMemcpyAsync(b.get(), h, nd, hipMemcpyHostToDevice, stream()));
        sync();
    }
    u8* p() { return b.get(); }
};
// esuf, ephr, ebw (alloc entries): in/out
KP int kp_entry_info(const u32* sa_d, const u64* dinfo, const u8* dict, u32 nd, int pack_prev, u32* esuf, u32* ephr, u8* ebw,
                     u32 alloc) {
    return guarded([&] {
        need(alloc >= nd, "the columns hold nd entries");
        for (u32 r = 0; r < nd; r++) need(sa_d[r] < nd, "sa_d beyond the dictionary");
        Dev<u32> sa(sa_d, nd), es(esuf, alloc), ep(ephr, alloc);
        Dev<u64> di(dinfo, nd);
        Dev<u8> eb(ebw, alloc);
        DevDict d(dict, nd);
        pk::entry_info(sa.p(), di.p(), d.p(), nd, pack_prev != 0, es.p(), ep.p(), eb.p(), stream());
        es.down(esuf); ep.down(ephr); eb.down(ebw);
    });
}
static void check_dict_entries(const u32* sa_d, const u32* esuf, u32 nd) {
    for (u32 r = 0; r < nd; r++) need(sa_d[r] < nd && (u64)sa_d[r] + (esuf[r] & 0x7fffffffu) <= nd, "a phrase suffix beyond the dictionary");
}
// plcp (nd entries): out; longs (4 * long_alloc words), long_count: in/out
KP int kp_dict_irreducible(const u8* dict, u32 nd, const u32* sa_d, const u32* esuf, const u8* ebw, u32* plcp, u32* longs,
                           u32 long_alloc, u32* long_count, u32 long_cap) {
    return guarded([&] {
        need(long_cap <= long_alloc, "long_cap beyond the list");
        check_dict_entries(sa_d, esuf, nd);
        DevDict d(dict, nd);
        Dev<u32> sa(sa_d, nd), es(esuf, nd), pl(nullptr, nd), lg(longs, 4 * (size_t)long_alloc), lc(long_count, 1);
        Dev<u8> eb(ebw, nd);
        pk::dict_irreducible(d.p(), nd, sa.p(), es.p(), eb.p(), pl.p(), lg.p(), lc.p(), long_cap, stream());
        pl.down(plcp); lg.down(longs); lc.down(long_count);
    });
}
// longs: count records (p, q, h, lim); plcp (nd entries): in/out
KP int kp_long_lcp_lim(const u8* dict, u32 nd, const u32* longs, u32 count, u32* plcp) {
    return guarded([&] {
        for (u32 i = 0; i < count; i++) {
            const u32* r = longs + 4 * (size_t)i;
            need(r[0] < nd && r[1] < nd && (u64)std::max(r[0], r[1]) + r[3] <= nd && r[2] <= r[3], "a record beyond the dictionary");
        }
        DevDict d(dict, nd);
        Dev<u32> lg(longs, 4 * (size_t)count), pl(plcp, nd), huge(nullptr, (size_t)count + 1), hc(nullptr, 1);
        k::long_lcp_lim(d.p(), nd, lg.p(), count, pl.p(), huge.p(), hc.p(), stream());
        pl.down(plcp);
    });
}
KP int kp_plcp_running_max(u32* plcp, u32 n, u32 alloc) {                                    // plcp (alloc entries): in/out
    return guarded([&] {
        need(alloc >= n, "plcp holds n entries");
        Dev<u32> pl(plcp, alloc);
        Dev<u8> scratch(nullptr, k::plcp_running_max_scratch(n));
        k::plcp_running_max(pl.p(), n, scratch.p(), stream());
        pl.down(plcp);
    });
}
KP int kp_lcp_gather(const u32* plcp, u32 n, const u32* sa, u32 count, u32* lcp, u32 alloc) {   // lcp (alloc entries): in/out
    return guarded([&] {
        need(alloc >= count, "lcp holds count entries");
        for (u32 j = 0; j < count; j++) need(sa[j] < n, "sa beyond plcp");
        Dev<u32> pl(plcp, n), a(sa, count), o(lcp, alloc);
        SaCol col; col.lo = a.p(); col.hi = nullptr;
        k::lcp_gather(pl.p(), col, 0, count, o.p(), stream());
        o.down(lcp);
    });
}
KP int kp_dict_lcp_clamp(u32* lcp, const u32* esuf, u32 nd, u32 alloc) {                     // lcp (alloc entries): in/out
    return guarded([&] {
        need(alloc >= nd, "lcp holds nd entries");
        Dev<u32> l(lcp, alloc), es(esuf, nd);
        pk::dict_lcp_clamp(l.p(), es.p(), nd, stream());
        l.down(lcp);
    });
}

// ---- A3: groups, ranks ------------------------------------------------------------------------------------------------
// gflag, pflag, vflag, seg (alloc entries): in/out
KP int kp_group_flags(const u32* esuf, const u32* lcp_d, u32 nd, u32 w, u32* gflag, u32* pflag, u32* vflag, u64* seg, u32 alloc) {
    return guarded([&] {
        need(alloc >= nd, "the columns hold nd entries");
        Dev<u32> es(esuf, nd), l(lcp_d, nd), g(gflag, alloc), p(pflag, alloc), v(vflag, alloc);
        Dev<u64> sg(seg, alloc);
        pk::group_flags(es.p(), l.p(), nd, w, g.p(), p.p(), v.p(), sg.p(), stream());
        g.down(gflag); p.down(pflag); v.down(vflag); sg.down(seg);
    });
}
KP int kp_phrase_ranks(const u32* esuf, const u32* ephr, const u32* pscan, u32 nd, u32* prank, u32 alloc) {     // prank: in/out
    return guarded([&] {
        for (u32 r = 0; r < nd; r++) need(!(esuf[r] >> 31) || ephr[r] < alloc, "ephr beyond prank");
        Dev<u32> es(esuf, nd), ep(ephr, nd), ps(pscan, nd), pr(prank, alloc);
        pk::phrase_ranks(es.p(), ep.p(), ps.p(), nd, pr.p(), stream());
        pr.down(prank);
    });
}
KP int kp_parse_ranks(const u32* pid, const u32* prank, u32 n_distinct, u32 m, u32* parse, u32 alloc) {          // parse: in/out
    return guarded([&] {
        need(alloc >= m, "parse holds m entries");
        for (u32 q = 0; q < m; q++) need(pid[q] < n_distinct, "pid beyond prank");
        Dev<u32> pi(pid, m), pr(prank, n_distinct), o(parse, alloc);
        pk::parse_ranks(pi.p(), pr.p(), m, o.p(), stream());
        o.down(parse);
    });
}
KP int kp_invert_ranks(const u32* prank, const u32* rep, const u32* dlen, u32 n_distinct, u32* which, u32* slen, u32 alloc) {
    return guarded([&] {
        for (u32 d = 0; d < n_distinct; d++) need(prank[d] >= 1 && prank[d] <= alloc, "prank is 1 .. alloc");
        Dev<u32> pr(prank, n_distinct), r(rep, n_distinct), dl(dlen, n_distinct), wh(which, alloc), sl(slen, alloc);
        pk::invert_ranks(pr.p(), r.p(), dl.p(), n_distinct, wh.p(), sl.p(), stream());
        wh.down(which); sl.down(slen);
    });
}

// ---- A4: inverted lists and emitter tables ----------------------------------------------------------------------------
KP int kp_occ_sequence(const u32* sa_p, const u32* pid, u32 m, u32 D, u32* keys, u32* vals, u32 alloc) {         // keys, vals: in/out
    return guarded([&] {
        need(m >= 1 && alloc >= (u64)m + 1, "keys / vals hold m + 1 entries");
        for (u32 r = 0; r < m; r++) need(sa_p[r] < m, "sa_p beyond the parse");
        Dev<u32> sa(sa_p, m), pi(pid, m), kk(keys, alloc), vv(vals, alloc);
        pk::occ_sequence(sa.p(), pi.p(), m, D, kk.p(), vv.p(), stream());
        kk.down(keys); vv.down(vals);
    });
}
static void check_occ(const u32* ids, const u32* ts, const u32* sa_p, u32 m, u32 start_alloc) {
    need(m >= 1, "m >= 1");
    for (u32 k = 0; k <= m; k++) need(ids[k] < start_alloc, "ids beyond occ_start");
    for (u32 k = 0; k < m; k++) need(ts[k] <= m && (ts[k] == 0 || (sa_p[ts[k] - 1] >= 1 && sa_p[ts[k] - 1] <= m)), "ts / sa_p out of range (the parse's first suffix belongs to the dummy, entry m)");
}
// mode 8: occ_finish (occ: m records of 8 bytes, occ_sl); mode 12: occ_finish12 (occ: m records of 12 bytes).
// occ_start (start_alloc), occ (occ_alloc records), occ_sl (occ_alloc): in/out
KP int kp_occ_finish(int mode, const u32* ids, const u32* ts, const u32* sa_p, const void* pstart, int wide, u32 m, u32* occ_start,
                     u32 start_alloc, void* occ, u32 occ_alloc, u32 pos_bits, const u32* sl, u32* occ_sl) {
    return guarded([&] {
        need(mode == 8 || mode == 12, "mode 8 or 12");
        need(occ_alloc >= m && (mode == 12 || pos_bits < 64), "occ holds m records");
        check_occ(ids, ts, sa_p, m, start_alloc);
        Dev<u32> i(ids, (size_t)m + 1), t(ts, (size_t)m + 1), sa(sa_p, m), os(occ_start, start_alloc), s(sl, m),
            osl(occ_sl, mode == 8 ? occ_alloc : 0);
        DevPos ps(pstart, m, wide != 0);
        Dev<u8> o((const u8*)occ, (size_t)occ_alloc * mode);
        if (mode == 8)
            pk::occ_finish(i.p(), t.p(), sa.p(), ps.p(), m, os.p(), (u64*)o.p(), pos_bits, s.p(), osl.p(), wide != 0, stream());
        else
            pk::occ_finish12(i.p(), t.p(), sa.p(), ps.p(), wide != 0, m, os.p(), (u32*)o.p(), s.p(), stream());
        os.down(occ_start); o.down((u8*)occ); osl.down(occ_sl);
    });
}
KP int kp_phrase_table(const u32* occ_start, const u32* plen, u32 n_plen, const u32* rep, u32 D, u32* tab, u32 alloc) {   // tab (4 * alloc words): in/out
    return guarded([&] {
        need(alloc >= D, "tab holds n_distinct records");
        for (u32 d = 0; d < D; d++) need(rep[d] < n_plen, "rep beyond plen");
        Dev<u32> os(occ_start, (size_t)D + 1), pl(plen, n_plen), r(rep, D), tb(tab, 4 * (size_t)alloc);
        pk::phrase_table(os.p(), pl.p(), r.p(), D, tb.p(), stream());
        tb.down(tab);
    });
}
// the compact columns (e_alloc entries each): in/out
KP int kp_entry_compact(const u32* esuf, const u32* ephr, const u8* ebw, const u32* gflag, const u32* gscan, const u32* vflag,
                        const u32* vscan, const u64* segmin, const u32* tab, u32 D, u32 nd, u32 e_alloc, u32* ce_cnt,
                        u32* ce_first, u32* ce_offm1, u8* ce_bwt, u32* ce_gs, u32* ce_hl, u32* ce_slen) {
    return guarded([&] {
        for (u32 r = 0; r < nd; r++) need(!vflag[r] || (vscan[r] < e_alloc && ephr[r] < D), "vscan / ephr out of range");
        Dev<u32> es(esuf, nd), ep(ephr, nd), gf(gflag, nd), gs(gscan, nd), vf(vflag, nd), vs(vscan, nd), tb(tab, 4 * (size_t)D),
            c0(ce_cnt, e_alloc), c1(ce_first, e_alloc), c2(ce_offm1, e_alloc), c4(ce_gs, e_alloc), c5(ce_hl, e_alloc),
            c6(ce_slen, e_alloc);
        Dev<u8> eb(ebw, nd), c3(ce_bwt, e_alloc);
        Dev<u64> sm(segmin, nd);
        pk::entry_compact(es.p(), ep.p(), eb.p(), gf.p(), gs.p(), vf.p(), vs.p(), sm.p(), tb.p(), nd, c0.p(), c1.p(), c2.p(),
                          c3.p(), c4.p(), c5.p(), c6.p(), stream());
        c0.down(ce_cnt); c1.down(ce_first); c2.down(ce_offm1); c3.down(ce_bwt); c4.down(ce_gs); c5.down(ce_hl); c6.down(ce_slen);
    });
}
KP int kp_group_heads(const u32* sege, const u32* ce_hl, const u32* ce_slen, u32 n_entries, u32 n_groups, u32* ghead, u32 alloc) {
    return guarded([&] {
        need(alloc >= n_groups, "ghead holds n_groups pairs");
        for (u32 g = 0; g < n_groups; g++) need(sege[g] < n_entries && (g == 0 || sege[g] >= 1), "sege out of range");
        Dev<u32> sg(sege, n_groups), hl(ce_hl, n_entries), sl(ce_slen, n_entries), gh(ghead, 2 * (size_t)alloc);
        pk::group_heads(sg.p(), hl.p(), sl.p(), n_groups, gh.p(), stream());
        gh.down(ghead);
    });
}
// out (alloc entries): in/out; segb: n_groups entries
KP int kp_tile_first(const void* segb, u32 n_groups, u64 tiles, u32* out, u32 alloc, int wide, u64 tile_base) {
    return guarded([&] {
        const u64 tile = pk::emit_tile();
        need(tiles >= tile_base && tiles - tile_base + 1 <= alloc, "out holds tiles - tile_base + 1 entries");
        for (u32 g = 0; g < n_groups; g++) {
            need(pos_at(segb, wide != 0, g) / tile + 1 >= tile_base, "a group before the table's first tile");
            need(g == 0 || pos_at(segb, wide != 0, g) >= pos_at(segb, wide != 0, g - 1), "segb ascends");
        }
        DevPos sb(segb, n_groups, wide != 0);
        Dev<u32> o(out, alloc);
        pk::tile_first(sb.p(), n_groups, tiles, o.p(), wide != 0, stream(), tile_base);
        o.down(out);
    });
}
// segb: n_groups + 1 entries; osize (alloc entries), err (16 words): in/out
KP int kp_oversize(const void* segb, u32 n_groups, u32* osize, u32 alloc, u32* err, int wide) {
    return guarded([&] {
        need(alloc >= n_groups, "osize holds n_groups entries");
        DevPos sb(segb, (size_t)n_groups + 1, wide != 0);
        Dev<u32> o(osize, alloc), e(err, 16);
        pk::oversize(sb.p(), n_groups, o.p(), e.p(), wide != 0, stream());
        o.down(osize); e.down(err);
    });
}
KP int kp_gather_pos(const void* src, u32 n_src, const u32* idx, u32 n, void* out, u32 alloc, int wide) {        // out: in/out
    return guarded([&] {
        need(alloc >= n, "out holds n entries");
        for (u32 i = 0; i < n; i++) need(idx[i] < n_src, "idx beyond src");
        DevPos s(src, n_src, wide != 0), o(out, alloc, wide != 0);
        Dev<u32> ix(idx, n);
        pk::gather_pos(s.p(), ix.p(), n, o.p(), wide != 0, stream());
        o.down(out);
    });
}
KP int kp_relative_offsets(const void* fb_off, u32 n_off, u32 f0, u32 count, u32* rel, u32 alloc, int wide) {    // rel: in/out
    return guarded([&] {
        need((u64)f0 + count < n_off && alloc >= (u64)count + 1, "fb_off[f0 .. f0 + count] and rel[0 .. count]");
        DevPos f(fb_off, n_off, wide != 0);
        Dev<u32> r(rel, alloc);
        pk::relative_offsets(f.p(), f0, count, r.p(), wide != 0, stream());
        r.down(rel);
    });
}
KP int kp_iota(u32* out, u32 n, u32 alloc) {                                                 // out: in/out
    return guarded([&] {
        need(alloc >= n, "out holds n entries");
        Dev<u32> o(out, alloc);
        pk::iota(o.p(), n, stream());
        o.down(out);
    });
}
KP int kp_gather_u64(const u64* src, u32 n_src, const u32* idx, u32 n, u64* out, u32 alloc) {                    // out: in/out
    return guarded([&] {
        need(alloc >= n, "out holds n entries");
        for (u32 i = 0; i < n; i++) need(idx[i] < n_src, "idx beyond src");
        Dev<u64> s(src, n_src), o(out, alloc);
        Dev<u32> ix(idx, n);
        pk::gather_u64(s.p(), ix.p(), n, o.p(), stream());
        o.down(out);
    });
}

// ---- parse_lcp.hpp ----------------------------------------------------------------------------------------------------
// bmin (alloc entries): receives levels * nb entries; dims = (nb, levels)
KP int kp_build_rmq(const u32* vals, u32 m, u32* bmin, u32 alloc, u32* dims) {
    return guarded([&] {
        need(m >= 1, "m >= 1");
        Dev<u32> v(vals, m);
        DevBuf<u32> b;
        u32 nb = 0, levels = 0;
        build_rmq(v.p(), m, b, nb, levels, stream());
        sync();
        need((u64)nb * levels <= alloc, "bmin holds levels * nb entries");
        MMT_HIP(hipMemcpyAsync(bmin, b.get(), (size_t)nb * levels * 4, hipMemcpyDeviceToHost, stream()));
        dims[0] = nb; dims[1] = levels;
    });
}
// The one kernel of the probe: rmq_min and rmq_min8 are __device__ inlines without a host wrapper; it only calls them.
__global__ void k_probe_rmq(RmqView R, const u32* __restrict__ ab, u32 n_pairs, u32* __restrict__ out, u32* __restrict__ out8) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pairs) return;
    out[i] = rmq_min(R, ab[2 * i], ab[2 * i + 1]);
    out8[i] = rmq_min8(R, ab[2 * i], ab[2 * i + 1]);
}
// ab: n_pairs pairs (a, b), a <= b < m; the view is the one build_rmq makes of vals inside this call
KP int kp_rmq_query(const u32* vals, u32 m, const u32* ab, u32 n_pairs, u32* out, u32* out8) {
    return guarded([&] {
        need(m >= 1, "m >= 1");
        for (u32 i = 0; i < n_pairs; i++) need(ab[2 * i] <= ab[2 * i + 1] && ab[2 * i + 1] < m, "a <= b < m");
        Dev<u32> v(vals, m), q(ab, 2 * (size_t)n_pairs), o(nullptr, n_pairs), o8(nullptr, n_pairs);
        DevBuf<u32> b;
        RmqView R;
        R.sl = v.p(); R.m = m;
        u32 levels = 0;
        build_rmq(v.p(), m, b, R.nb, levels, stream());
        R.bmin = b.get();
        if (n_pairs) {
            hipLaunchKernelGGL(k_probe_rmq, dim3((n_pairs + 255) / 256), dim3(256), 0, stream(), R, q.p(), n_pairs, o.p(), o8.p());
            MMT_HIP(hipGetLastError());
        }
        o.down(out); o8.down(out8);
    });
}
// sl (m entries), bmin (alloc entries; levels * nb come back); dims = (nb, levels, n_irreducible, n_long)
KP int kp_parse_lcp(const KpText* tx, u64 nv, const u32* sa_p, const u32* pid, const void* pstart, int wide, u32 m, u32* sl,
                    u32* bmin, u32 alloc, u32* dims) {
    return guarded([&] {
        need(m >= 1, "m >= 1");
        DevText t(tx);
        need(nv <= t.readable && nv >= 1, "nv within V");
        for (u32 r = 0; r < m; r++) need(sa_p[r] < m && pos_at(pstart, wide != 0, r) < nv, "sa_p / pstart out of range");
        Dev<u32> sa(sa_p, m), pi(pid, m);
        DevPos ps(pstart, m, wide != 0);
        Dev<u8> temp(nullptr, 0);
        ParseLcp L;
        L.build(t.T, nv, sa.p(), pi.p(), ps.p(), wide != 0, m, temp.b, stream());
        sync();
        need((u64)L.nb * L.levels <= alloc, "bmin holds levels * nb entries");
        MMT_HIP(hipMemcpyAsync(sl, L.sl.get(), (size_t)m * 4, hipMemcpyDeviceToHost, stream()));
        MMT_HIP(hipMemcpyAsync(bmin, L.bmin.get(), (size_t)L.nb * L.levels * 4, hipMemcpyDeviceToHost, stream()));
        dims[0] = L.nb; dims[1] = L.levels; dims[2] = L.n_irreducible; dims[3] = L.n_long;
    });
}

// ==== guided_kernels.hpp (mmt::gk): the bucket-wise producer's wrappers, kp_gk_<wrapper> ================================
// The model of these kernels is tests/guidedmodel.py, their cases tests/guided_cases.py (which mirrors the need(...) lines
// below, so that the CPU suite knows that no designed case is rejected here).
static u32 popc64(u64 x) { return (u32)__builtin_popcountll(x); }
// ---- phrase-end tables ------------------------------------------------------------------------------------------------
// counts (alloc entries): in/out
KP int kp_gk_rank_counts(const u64* mask, u64 n_words, u32* counts, u64 n_counts, u32 alloc) {
    return guarded([&] {
        need(alloc >= n_counts, "counts holds n_counts entries");
        Dev<u64> m(mask, n_words);
        Dev<u32> c(counts, alloc);
        gk::rank_counts(m.p(), n_words, c.p(), n_counts, stream());
        c.down(counts);
    });
}
KP int kp_gk_block_first_cut(const u64* mask, u64 n_words, u64* first, u64 n_blocks, u32 alloc) {      // first: in/out
    return guarded([&] {
        need(alloc >= n_blocks, "first holds n_blocks entries");
        Dev<u64> m(mask, n_words), f(first, alloc);
        gk::block_first_cut(m.p(), n_words, f.p(), n_blocks, stream());
        f.down(first);
    });
}
KP int kp_gk_block_cut_counts(const u64* mask, u64 n_words, u32* counts, u64 n_blocks, u32 alloc) {    // counts: in/out
    return guarded([&] {
        need(alloc >= n_blocks, "counts holds n_blocks entries");
        Dev<u64> m(mask, n_words);
        Dev<u32> c(counts, alloc);
        gk::block_cut_counts(m.p(), n_words, c.p(), n_blocks, stream());
        c.down(counts);
    });
}
// brank: n_blocks entries; coff (alloc entries): in/out
KP int kp_gk_block_cut_offsets(const u64* mask, u64 n_words, const u32* brank, uint16_t* coff, u64 n_blocks, u32 alloc) {
    return guarded([&] {
        for (u64 b = 0; b < n_blocks; b++) {
            u64 c = 0;
            for (u64 wi = b * 64; wi < std::min<u64>(n_words, (b + 1) * 64); wi++) c += popc64(mask[wi]);
            need((u64)brank[b] + c <= alloc, "brank + the block's cuts beyond coff");
        }
        Dev<u64> m(mask, n_words);
        Dev<u32> br(brank, n_blocks);
        Dev<uint16_t> co(coff, alloc);
        gk::block_cut_offsets(m.p(), n_words, br.p(), co.p(), n_blocks, stream());
        co.down(coff);
    });
}

// ---- staged lists (the context-free half) -------------------------------------------------------------------------------
// tile_off: n_tiles entries; blk_tile (alloc entries): in/out
KP int kp_gk_stage_block_tiles(const u32* tile_off, u32 n_tiles, u64 n, u32* blk_tile, u32 alloc) {
    return guarded([&] {
        need(n_tiles >= 1 && n < (1ull << 32), "n_tiles >= 1, a list below 2^32 entries");
        need(n == 0 || alloc >= (n + 4095) / 4096 + 1, "blk_tile holds blocks + 1 entries");
        Dev<u32> to(tile_off, n_tiles), bt(blk_tile, alloc);
        gk::stage_block_tiles(to.p(), n_tiles, n, bt.p(), stream());
        bt.down(blk_tile);
    });
}
KP int kp_gk_stage_count(const u32* staged, u64 n, u32 b0, u32 b1, u32* block_count, u32 alloc) {     // block_count: in/out
    return guarded([&] {
        need(alloc >= (n + 4095) / 4096, "block_count holds one entry per 4096 entries");
        Dev<u32> st(staged, n), bc(block_count, alloc);
        gk::stage_count(st.p(), n, b0, b1, bc.p(), stream());
        bc.down(block_count);
    });
}

// ---- first keys and rounds ------------------------------------------------------------------------------------------
// head, active (alloc entries), lcp (alloc entries, or null): in/out
KP int kp_gk_heads0(const u64* keys, u32 B, u8* head, u8* active, u32* lcp, u32 alloc, int bits, int chars) {
    return guarded([&] {
        need(alloc >= B && bits >= 1 && chars >= 1 && bits * chars <= 64, "B entries, 1 <= bits * chars <= 64");
        Dev<u64> k(keys, B);
        Dev<u8> h(head, alloc), a(active, alloc);
        Dev<u32> l(lcp, lcp ? alloc : 0);
        gk::heads0(k.p(), B, h.p(), a.p(), lcp ? l.p() : nullptr, bits, chars, stream());
        h.down(head); a.down(active); l.down(lcp);
    });
}
// pos_sorted, head: B entries; slot, pos, headval (alloc entries): in/out
KP int kp_gk_gather_active(const u32* idx, u32 m, const u64* pos_sorted, const u8* head, u32 B, u32* slot, u64* pos, u32* headval,
                           u32 alloc) {
    return guarded([&] {
        need(alloc >= m, "the outputs hold m entries");
        for (u32 c = 0; c < m; c++) need(idx[c] < B, "idx beyond the batch");
        Dev<u32> i(idx, m), sl(slot, alloc), hv(headval, alloc);
        Dev<u64> ps(pos_sorted, B), po(pos, alloc);
        Dev<u8> h(head, B);
        gk::gather_active(i.p(), m, ps.p(), h.p(), sl.p(), po.p(), hv.p(), stream());
        sl.down(slot); po.down(pos); hv.down(headval);
    });
}
// group heads of a list of m elements: ghead[c] = index of the first element of c's group
static void check_gheads(const u32* ghead, u32 m) {
    for (u32 c = 0; c < m; c++) need(ghead[c] == c || (c > 0 && ghead[c] == ghead[c - 1] && ghead[c] < c), "ghead: every element names the first of its group");
}
// list (2 * alloc words: pairs, 4 regions of cap), count4 (count_alloc >= 4 words): in/out
KP int kp_gk_medium_groups(const u32* ghead, u32 m, u32* list, u32 cap, u32 alloc, u32* count4, u32 count_alloc) {
    return guarded([&] {
        check_gheads(ghead, m);
        need(count_alloc >= 4 && alloc >= 4 * (u64)cap, "count4 holds 4 words, list 4 regions of cap pairs");
        u32 cnt[4] = {0, 0, 0, 0};
        for (u32 e = 0; e < m; e++)
            if (e + 1 == m || ghead[e + 1] != ghead[e]) {
                const u32 sz = e - ghead[e] + 1;
                if (sz <= 128) cnt[sz <= 16 ? 0 : (sz <= 32 ? 1 : (sz <= 64 ? 2 : 3))]++;
            }
        for (int cl = 0; cl < 4; cl++) need(cnt[cl] <= cap, "a class has more groups than a region holds");
        Dev<u32> g(ghead, m), l(list, 2 * (size_t)alloc), c4(count4, count_alloc);
        gk::medium_groups(g.p(), m, l.p(), cap, c4.p(), stream());
        l.down(list); c4.down(count4);
    });
}
KP int kp_gk_tile_bounds(const u32* ghead, u32 m, u32 target, u32 limit, u32 n_tiles, u32* bound, u32 alloc) {    // bound: in/out
    return guarded([&] {
        need(alloc >= (u64)n_tiles + 1 && target >= 1, "bound holds n_tiles + 1 entries");
        Dev<u32> g(ghead, m), b(bound, alloc);
        gk::tile_bounds(g.p(), m, target, limit, n_tiles, b.p(), stream());
        b.down(bound);
    });
}
// kout, pout (m entries), big_begin, big_end (big_alloc entries), big_count: in/out
KP int kp_gk_local_sort(const u64* kin, const u64* pin, const u32* ghead, u32 m, u64* kout, u64* pout, const u32* bound, u32 n_tiles,
                        u32* big_begin, u32* big_end, u32 big_alloc, u32* big_count, u32 big_cap) {
    return guarded([&] {
        need(big_cap <= big_alloc && n_tiles >= 1, "big_cap within the lists, a tile at least");
        check_gheads(ghead, m);
        need(bound[n_tiles] != gk::NO_BOUND, "the last bound ends every search");
        for (u32 t = 0; t <= n_tiles; t++)
            need(bound[t] == gk::NO_BOUND || (bound[t] <= m && (bound[t] == m || ghead[bound[t]] == bound[t])), "a bound is a group's head or m");
        Dev<u64> ki(kin, m), pi(pin, m), ko(kout, m), po(pout, m);
        Dev<u32> g(ghead, m), b(bound, (size_t)n_tiles + 1), bb(big_begin, big_alloc), be(big_end, big_alloc), bc(big_count, 1);
        gk::local_sort(ki.p(), pi.p(), g.p(), ko.p(), po.p(), b.p(), n_tiles, bb.p(), be.p(), bc.p(), big_cap, stream());
        ko.down(kout); po.down(pout); bb.down(big_begin); be.down(big_end); bc.down(big_count);
    });
}
// seg_begin, seg_end (seg_alloc entries), seg_count (count_alloc >= 1 entries): in/out
KP int kp_gk_range_groups(const u32* ghead, u32 m, const u32* big_begin, const u32* big_end, u32 big, u32* seg_begin, u32* seg_end,
                          u32 seg_alloc, u32* seg_count, u32 count_alloc) {
    return guarded([&] {
        need(big >= 1 && count_alloc >= 1, "a range at least");
        check_gheads(ghead, m);
        u64 segs = 0;
        for (u32 r = 0; r < big; r++) {
            need(big_begin[r] <= big_end[r] && big_end[r] <= m, "a range within the list");
            for (u32 c = big_begin[r]; c < big_end[r]; c++) segs += (c + 1 == big_end[r] || ghead[c + 1] == c + 1) ? 1 : 0;
        }
        need(segs <= seg_alloc, "more groups than the segment lists hold");
        Dev<u32> g(ghead, m), bb(big_begin, big), be(big_end, big), sb(seg_begin, seg_alloc), se(seg_end, seg_alloc), sc(seg_count, count_alloc);
        gk::range_groups(g.p(), bb.p(), be.p(), big, sb.p(), se.p(), sc.p(), stream());
        sb.down(seg_begin); se.down(seg_end); sc.down(seg_count);
    });
}
// out (out_alloc entries), flags (alloc entries): in/out
KP int kp_gk_round_apply(const u64* pos_sorted, const u32* newhead, const u32* slot, u32 m, u64* out, u32 out_alloc, u8* flags, u32 alloc) {
    return guarded([&] {
        need(alloc >= m, "flags holds m entries");
        for (u32 c = 0; c < m; c++) need(slot[c] < out_alloc, "slot beyond out");
        Dev<u64> ps(pos_sorted, m), o(out, out_alloc);
        Dev<u32> nh(newhead, m), sl(slot, m);
        Dev<u8> f(flags, alloc);
        gk::round_apply(ps.p(), nh.p(), sl.p(), m, o.p(), f.p(), stream());
        o.down(out); f.down(flags);
    });
}
// slot, pos_sorted, newhead: m entries; the outputs (alloc entries): in/out
KP int kp_gk_round_compact(const u32* idx, u32 m2, const u32* slot, const u64* pos_sorted, const u32* newhead, u32 m, u32* slot_out,
                           u64* pos_out, u32* headval_out, u32 alloc) {
    return guarded([&] {
        need(alloc >= m2, "the outputs hold m2 entries");
        for (u32 c = 0; c < m2; c++) need(idx[c] < m, "idx beyond the round's list");
        Dev<u32> i(idx, m2), sl(slot, m), nh(newhead, m), so(slot_out, alloc), ho(headval_out, alloc);
        Dev<u64> ps(pos_sorted, m), po(pos_out, alloc);
        gk::round_compact(i.p(), m2, sl.p(), ps.p(), nh.p(), so.p(), po.p(), ho.p(), stream());
        so.down(slot_out); po.down(pos_out); ho.down(headval_out);
    });
}

// ---- giant bookkeeping ------------------------------------------------------------------------------------------------
KP int kp_gk_flag_greater(const u32* v, u32 n, u32 thr, u32* flags, u32 alloc) {              // flags: in/out
    return guarded([&] {
        need(alloc >= n, "flags holds n entries");
        Dev<u32> a(v, n), f(flags, alloc);
        gk::flag_greater(a.p(), n, thr, f.p(), stream());
        f.down(flags);
    });
}
KP int kp_gk_flag_spread(const u32* in, u32 n, u32* out, u32 alloc) {                         // out: in/out
    return guarded([&] {
        need(alloc >= n, "out holds n entries");
        Dev<u32> a(in, n), o(out, alloc);
        gk::flag_spread(a.p(), n, o.p(), stream());
        o.down(out);
    });
}
KP int kp_gk_flag_to_distinct(const u32* occ_flag, const u32* pid, u32 m, u32* dflag, u32 alloc) {   // dflag: in/out
    return guarded([&] {
        for (u32 k = 0; k < m; k++) need(pid[k] < alloc, "pid beyond dflag");
        Dev<u32> of(occ_flag, m), pi(pid, m), d(dflag, alloc);
        gk::flag_to_distinct(of.p(), pi.p(), m, d.p(), stream());
        d.down(dflag);
    });
}
KP int kp_gk_flag_from_distinct(const u32* dflag, u32 D, const u32* pid, u32 m, u32* occ_flag, u32 alloc) {   // occ_flag: in/out
    return guarded([&] {
        need(alloc >= m, "occ_flag holds m entries");
        for (u32 k = 0; k < m; k++) need(pid[k] < D, "pid beyond dflag");
        Dev<u32> d(dflag, D), pi(pid, m), of(occ_flag, alloc);
        gk::flag_from_distinct(d.p(), pi.p(), m, of.p(), stream());
        of.down(occ_flag);
    });
}
KP int kp_gk_flag_scatter_ones(const u32* ids, u32 n, u32* flags, u32 alloc) {                // flags: in/out
    return guarded([&] {
        for (u32 i = 0; i < n; i++) need(ids[i] < alloc, "ids beyond flags");
        Dev<u32> a(ids, n), f(flags, alloc);
        gk::flag_scatter_ones(a.p(), n, f.p(), stream());
        f.down(flags);
    });
}
KP int kp_gk_giant_distinct(const u32* gids, u32 n, const u32* rep, const u32* dlen, u32 D, u32* which, u32* glen, u32 alloc) {
    return guarded([&] {
        need(alloc >= n, "which / glen hold n entries");
        for (u32 i = 0; i < n; i++) need(gids[i] < D, "gids beyond rep / dlen");
        Dev<u32> g(gids, n), r(rep, D), dl(dlen, D), wh(which, alloc), gl(glen, alloc);
        gk::giant_distinct(g.p(), n, r.p(), dl.p(), wh.p(), gl.p(), stream());
        wh.down(which); gl.down(glen);
    });
}
KP int kp_gk_giant_bits(const u32* flags, u32 m, u32* bits, u32 alloc) {                      // bits: in/out
    return guarded([&] {
        need(alloc >= ((u64)m + 31) / 32, "bits holds a word per 32 flags");
        Dev<u32> f(flags, m), b(bits, alloc);
        gk::giant_bits(f.p(), m, b.p(), stream());
        b.down(bits);
    });
}
KP int kp_gk_popcount_words(const u32* bits, u32 n, u32* out, u32 alloc) {                    // out: in/out
    return guarded([&] {
        need(alloc >= n, "out holds n entries");
        Dev<u32> b(bits, n), o(out, alloc);
        gk::popcount_words(b.p(), n, o.p(), stream());
        o.down(out);
    });
}
KP int kp_gk_giant_map(const u32* gids, const u32* gstart, u32 n, u32* dmap, u32 alloc) {     // dmap: in/out
    return guarded([&] {
        for (u32 i = 0; i < n; i++) need(gids[i] < alloc, "gids beyond dmap");
        Dev<u32> g(gids, n), gs(gstart, n), d(dmap, alloc);
        gk::giant_map(g.p(), gs.p(), n, d.p(), stream());
        d.down(dmap);
    });
}
// pid, pstart: m entries; gps, gbase (alloc entries): in/out
KP int kp_gk_giant_occurrences(const u32* gk_, u32 n, const u32* pid, const void* pstart, int wide, u32 m, const u32* dmap, u32 D,
                               u64* gps, u32* gbase, u32 alloc) {
    return guarded([&] {
        need(alloc >= n, "gps / gbase hold n entries");
        for (u32 j = 0; j < n; j++) need(gk_[j] < m && pid[gk_[j]] < D, "gk beyond the parse, or pid beyond dmap");
        Dev<u32> g(gk_, n), pi(pid, m), dm(dmap, D), gb(gbase, alloc);
        DevPos ps(pstart, m, wide != 0);
        Dev<u64> gp(gps, alloc);
        gk::giant_occurrences(g.p(), n, pi.p(), ps.p(), wide != 0, dm.p(), gp.p(), gb.p(), stream());
        gp.down(gps); gb.down(gbase);
    });
}
KP int kp_gk_giant_group_flags(const u32* esuf, const u32* lcp, u32 nd, u32* flags, u32 alloc) {   // flags: in/out
    return guarded([&] {
        need(alloc >= nd, "flags holds nd entries");
        Dev<u32> es(esuf, nd), l(lcp, nd), f(flags, alloc);
        gk::giant_group_flags(es.p(), l.p(), nd, f.p(), stream());
        f.down(flags);
    });
}

// ---- results (the context-free half) ------------------------------------------------------------------------------------
KP int kp_gk_group_ids(u32* ce_gs, const u32* gscan, u32 B, u32 alloc) {                      // ce_gs: in/out
    return guarded([&] {
        need(alloc >= B, "ce_gs holds B entries");
        Dev<u32> g(ce_gs, alloc), sc(gscan, B);
        gk::group_ids(g.p(), sc.p(), B, stream());
        g.down(ce_gs);
    });
}
KP int kp_gk_add_offset(void* table, int wide, u32 n, u64 add, u32 alloc) {                   // table: in/out
    return guarded([&] {
        need(alloc >= n, "table holds n entries");
        DevPos t(table, alloc, wide != 0);
        gk::add_offset(t.p(), wide != 0, n, add, stream());
        t.down(table);
    });
}
KP int kp_gk_rep_bits(const u32* pid, const u32* rep, u32 D, u32 m, u32* bits, u32 alloc) {   // bits: in/out
    return guarded([&] {
        need(alloc >= ((u64)m + 31) / 32, "bits holds a word per 32 phrases");
        for (u32 k = 0; k < m; k++) need(pid[k] < D, "pid beyond rep");
        Dev<u32> pi(pid, m), r(rep, D), b(bits, alloc);
        gk::rep_bits(pi.p(), r.p(), m, b.p(), stream());
        b.down(bits);
    });
}

// ---- the context ------------------------------------------------------------------------------------------------------
// gk::Ctx field for field, every table a host pointer with its length (tile0 and prof are the wrappers' own business; acgt,
// acgt_lut and dense_ok come from gk::set_dense_codes as in guided.cpp, `no_dense` standing for the switch).  The phrase ends
// come as bits (mask + rdir) or as a list (coff + brank), never both.  g_lcp: the values g_rmq is built over.
struct KpCtx {
    const KpText* T; u64 n; u32 w;
    const u64* mask; u64 n_mask; const u32* rdir; u64 n_rdir; const u64* nxt; u64 n_nxt;
    const u32* isa_p; u32 m; const u8* code; int bits, chars; u32 skip, pos_bits, rec_rank; u32 no_dense;
    const u32* pid; const uint16_t* coff; u64 n_coff; const u32* brank; u64 n_brank;
    const u32* g_k; const u64* g_ps; const u32* g_base; u32 g_n; const u32* g_isa; const u32* g_grp; const u32* g_lcp; u32 n_gisa;
    u32 g_depth; const u32* g_bits; const u32* g_rank; const u32* repbits; u32 n_bitwords; u32 expand;
};
struct KpRunSlice { u32 sym, blo, bhi; const u64* lead; const u8* first; const u8* follow; u64 n_tiles; };

struct DevCtx {
    DevText t;
    Dev<u64> mask, nxt, g_ps;
    Dev<u32> rdir, isa_p, pid, brank, g_k, g_base, g_isa, g_grp, g_lcp, g_bits, g_rank, repbits;
    Dev<uint16_t> coff;
    Dev<u8> code;
    DevBuf<u32> g_bmin;
    gk::Ctx c;
    std::vector<u64> cuts;                      // the phrase ends the tables spell, for the checks of indices that depend on a rank
    u64 tiles;
    explicit DevCtx(const KpCtx* k)
        : t(k->T), mask(k->mask, k->mask ? k->n_mask : 0), nxt(k->nxt, k->n_nxt), g_ps(k->g_ps, k->g_n),
          rdir(k->rdir, k->rdir ? k->n_rdir : 0), isa_p(k->isa_p, k->isa_p ? k->m : 0), pid(k->pid, k->pid ? k->m : 0),
          brank(k->brank, k->brank ? k->n_brank : 0), g_k(k->g_k, k->g_n), g_base(k->g_base, k->g_n), g_isa(k->g_isa, k->n_gisa),
          g_grp(k->g_grp, k->n_gisa), g_lcp(k->g_lcp, k->n_gisa), g_bits(k->g_bits, k->g_n ? k->n_bitwords : 0),
          g_rank(k->g_rank, k->g_n ? k->n_bitwords : 0), repbits(k->repbits, k->repbits ? k->n_bitwords : 0),
          coff(k->coff, k->coff ? k->n_coff : 0), code(k->code, 256) {
        const u64 n = k->n, blocks = n / 4096 + 2;
        need(n >= 1 && n == k->T->n && k->w >= 1 && k->w <= 32, "n = text length >= 1, 1 <= w <= 32");
        need(k->bits >= 1 && k->chars >= 1 && k->bits * k->chars <= 63, "1 <= bits * chars <= 63");
        need(k->code && k->code[0] == 0 && k->nxt, "a code table (code[0] = 0) and nxt");
        need(k->pos_bits >= 1 && k->pos_bits <= 63 && (k->rec_rank || k->pos_bits == 40), "pos_bits 1 .. 63, 40 when the records carry lengths");
        need((k->mask && k->rdir && !k->coff && !k->brank) || (!k->mask && !k->rdir && k->coff && k->brank), "the phrase ends as bits or as a list");
        need(k->n_nxt >= blocks, "nxt holds n / 4096 + 2 entries");
        for (u64 b = 0; b < k->n_nxt; b++) need(k->nxt[b] <= n + k->w - 1, "nxt at most n + w - 1");
        if (k->mask) {
            need(k->n_mask >= blocks * 64 && k->n_rdir >= blocks * 8, "mask holds n / 4096 + 2 blocks of 64 words, rdir a count per 8 words");
            for (u64 wi = 0; wi < k->n_mask; wi++)
                for (u64 x = k->mask[wi]; x; x &= x - 1) cuts.push_back(wi * 64 + (u64)__builtin_ctzll(x));
        } else {
            need(k->n_brank >= blocks + 2, "brank holds n / 4096 + 4 entries");
            for (u64 b = 0; b + 1 < k->n_brank; b++) {
                need(k->brank[b] <= k->brank[b + 1] && k->brank[b + 1] <= k->n_coff, "brank ascends within coff");
                for (u32 e = k->brank[b]; e < k->brank[b + 1]; e++) {
                    need(k->coff[e] < 4096 && (e == k->brank[b] || k->coff[e] > k->coff[e - 1]), "coff ascends inside a block, below 4096");
                    cuts.push_back(b * 4096 + k->coff[e]);
                }
            }
        }
        need(cuts.empty() || cuts.back() < n, "phrase ends below n");
        need(k->m >= cuts.size() + 1, "m counts a phrase per phrase end and the last");
        need(k->isa_p || k->skip || k->expand, "isa_p unless the elements are phrases or representatives");
        need(k->n_bitwords >= ((u64)k->m + 31) / 32 || !(k->repbits || k->g_n), "a bit per phrase in repbits / g_bits");
        need(!k->g_n || (k->g_k && k->g_ps && k->g_base && k->g_isa && k->g_grp && k->g_lcp && k->g_bits && k->g_rank && k->n_gisa >= 1), "the giant tables");
        tiles = std::max<u64>(1, (n + 4095) / 4096);
        c.T = t.T; c.n = n; c.w = k->w; c.mask = k->mask ? mask.p() : nullptr; c.rdir = k->rdir ? rdir.p() : nullptr; c.nxt = nxt.p();
        c.isa_p = k->isa_p ? isa_p.p() : nullptr; c.m = k->m; c.code = code.p(); c.bits = k->bits; c.chars = k->chars;
        c.skip = k->skip; c.pos_bits = k->pos_bits; c.rec_rank = k->rec_rank;
        gk::set_dense_codes(c, k->code, k->no_dense != 0);
        c.pid = k->pid ? pid.p() : nullptr; c.coff = k->coff ? coff.p() : nullptr; c.brank = k->brank ? brank.p() : nullptr;
        c.repbits = k->repbits ? repbits.p() : nullptr; c.expand = k->expand; c.g_depth = k->g_depth; c.g_n = k->g_n;
        if (k->g_n) {
            c.g_k = g_k.p(); c.g_ps = g_ps.p(); c.g_base = g_base.p(); c.g_isa = g_isa.p(); c.g_grp = g_grp.p();
            c.g_bits = g_bits.p(); c.g_rank = g_rank.p();
            u32 levels = 0;
            c.g_rmq.sl = g_lcp.p(); c.g_rmq.m = k->n_gisa;
            build_rmq(g_lcp.p(), k->n_gisa, g_bmin, c.g_rmq.nb, levels, stream());
            c.g_rmq.bmin = g_bmin.get();
        }
    }
    // |alpha| of an element as the kernels read it: from the record, or from the phrase ends
    u64 len_of(const KpCtx* k, u64 rec) const {
        const u64 q = rec & ((1ull << k->pos_bits) - 1);
        const u64 len = rec >> 40;
        if (!k->rec_rank && len != gk::LEN_SAT) return len;
        const u64 x = q + k->skip + k->w - 2;
        const auto it = std::lower_bound(cuts.begin(), cuts.end(), x);
        return (x < c.n && it != cuts.end() ? *it : c.n + k->w - 1) + 2 - q;
    }
    // the giant tables as a whole: occurrence j is phrase g_k[j] (ascending, flagged in g_bits, counted by g_rank), begins at
    // g_ps[j], and its whole phrase lies inside the dictionary from g_base[j] on -- then every entry a comparison asks for
    // (an element of that phrase, a place before the end of its alpha) is inside g_isa; entries and groups inside the tables
    void check_giant_tables(const KpCtx* k) const {
        if (!k->g_n) return;
        u32 seen = 0;
        for (u32 ph = 0; ph < k->m; ph++) {
            const u32 word = k->g_bits[ph >> 5];
            if ((ph & 31) == 0) need(k->g_rank[ph >> 5] == seen, "g_rank counts the bits of g_bits");
            if (!((word >> (ph & 31)) & 1u)) continue;
            need(seen < k->g_n && k->g_k[seen] == ph, "g_k lists the phrases flagged in g_bits");
            const u64 start = ph == 0 ? 0 : cuts[ph - 1] - k->w + 2, end = ph < cuts.size() ? cuts[ph] + 1 : c.n + k->w;
            need(ph == 0 || cuts[ph - 1] + 2 >= k->w, "a phrase start inside V");
            need(k->g_ps[seen] == start && (u64)k->g_base[seen] + (end - start + 1) <= k->n_gisa, "a giant occurrence begins at its phrase and lies inside the dictionary");
            seen++;
        }
        need(seen == k->g_n, "g_n counts the flagged phrases");
        for (u32 r = 0; r < k->n_gisa; r++) need(k->g_isa[r] < k->n_gisa, "g_isa inside the dictionary");
    }
    // elements whose alphas are compared character by character: every character of alpha inside V (forged lengths too), the
    // shared prefix not longer than alpha, and giant tables that hold every entry a comparison may ask for
    void check_compared(const KpCtx* k, const u64* pos, u32 count, u64 offset) const {
        check_giant_tables(k);
        check_elements(k, pos, count);
        for (u32 e = 0; e < count; e++) {
            const u64 q = pos[e] & ((1ull << k->pos_bits) - 1), len = len_of(k, pos[e]);
            need(offset <= len && q + len <= c.n + 40, "alpha inside V, the shared prefix inside alpha");
        }
    }
    // the rank of the parse suffix behind an element, as rec_rank_key reads it
    u64 rank_key(const KpCtx* k, u64 rec) const {
        if (k->rec_rank) return rec >> k->pos_bits;
        const u32 ph = rank1((rec & ((1ull << k->pos_bits) - 1)) + k->skip + k->w - 2);
        return ph + 1 < k->m ? k->isa_p[ph + 1] : 0;
    }
    u32 rank1(u64 x) const { return (u32)(std::lower_bound(cuts.begin(), cuts.end(), std::min(x, c.n)) - cuts.begin()); }
    // every element of a list: a V index inside the text (1 .. n; a list of phrases may hold the first phrase, at 0)
    void check_elements(const KpCtx* k, const u64* pos, u32 count) const {
        for (u32 e = 0; e < count; e++) {
            const u64 q = pos[e] & ((1ull << k->pos_bits) - 1);
            need(q <= c.n && (q >= 1 || k->skip), "an element's V index is 1 .. n (0: the first phrase)");
        }
    }
};
struct DevRun {
    Dev<u64> lead; Dev<u8> first, follow;
    gk::RunSlice rs;
    DevRun(const KpRunSlice* r, u64 tiles)
        : lead(r ? r->lead : nullptr, r && r->sym ? r->n_tiles : 0), first(r ? r->first : nullptr, r && r->sym ? r->n_tiles : 0),
          follow(r ? r->follow : nullptr, r && r->sym ? r->n_tiles : 0) {
        if (!r || !r->sym) return;
        need(r->lead && r->first && r->follow && r->n_tiles <= tiles + 1, "a run slice names its three tables, a tile behind the text's last at most");
        need(r->blo <= r->bhi && r->bhi <= 2 * gk::RUN_BUCKETS_HALF, "buckets within 2 * RUN_BUCKETS_HALF");
        rs.sym = r->sym; rs.blo = r->blo; rs.bhi = r->bhi; rs.lead = lead.p(); rs.first = first.p(); rs.follow = follow.p(); rs.n_tiles = r->n_tiles;
    }
};
static void need_text_order(const KpCtx* k, int pc) {
    need(!k->skip && pc >= 1 && pc <= k->chars && k->bits * pc <= 20, "text suffixes; 1 <= prefix_chars <= chars, bins of at most 20 bits");
}

// ---- text-order kernels -----------------------------------------------------------------------------------------------------
// first, follow (alloc bytes), lead (alloc entries): in/out
KP int kp_gk_tile_lead(const KpCtx* k, u8* first, uint16_t* lead, u8* follow, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        need(!k->skip && alloc >= d.tiles, "text suffixes; the tables hold a tile each");
        Dev<u8> f(first, alloc), fo(follow, alloc);
        Dev<uint16_t> l(lead, alloc);
        gk::tile_lead(d.c, f.p(), l.p(), fo.p(), stream());
        f.down(first); l.down(lead); fo.down(follow);
    });
}
// hist (alloc entries): in/out, 4 * RUN_BUCKETS_HALF of them may be added to
KP int kp_gk_run_hist(const KpCtx* k, int pc, u32 bin, const KpRunSlice* r, u64* hist, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        need_text_order(k, pc);
        need(r && r->sym && alloc >= 4 * gk::RUN_BUCKETS_HALF, "a run slice; hist holds 4 * RUN_BUCKETS_HALF entries");
        DevRun dr(r, d.tiles);
        Dev<u64> h(hist, alloc);
        gk::run_hist(d.c, pc, bin, dr.rs, h.p(), stream());
        h.down(hist);
    });
}
KP int kp_gk_bin_hist(const KpCtx* k, int pc, u64* hist, u32 alloc) {                         // hist: in/out (added to)
    return guarded([&] {
        DevCtx d(k);
        need_text_order(k, pc);
        need(pc <= 5 && alloc >= (1u << (k->bits * pc)), "at most five leading characters; hist holds a counter per bin");
        Dev<u64> h(hist, alloc);
        gk::bin_hist(d.c, pc, h.p(), stream());
        h.down(hist);
    });
}
KP int kp_gk_batch_count(const KpCtx* k, int pc, u32 bin_lo, u32 bin_hi, const KpRunSlice* r, u32* tile_count, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        need_text_order(k, pc);
        need(alloc >= d.tiles, "tile_count holds a tile each");
        DevRun dr(r, d.tiles);
        Dev<u32> tc(tile_count, alloc);
        gk::batch_count(d.c, pc, bin_lo, bin_hi, tc.p(), stream(), dr.rs);
        tc.down(tile_count);
    });
}
// tile_off: a tile each; keys, pos (alloc entries), next_count (count_alloc entries, or null): in/out.  A tile selects 4096
// suffixes at the most: the lists must hold that many behind every tile's offset (what a tile does select is the kernel's answer).
KP int kp_gk_batch_fill(const KpCtx* k, int pc, u32 bin_lo, u32 bin_hi, const u32* tile_off, u64* keys, u64* pos, u32 alloc, u32 next_lo,
                        u32 next_hi, u32* next_count, u32 count_alloc, const KpRunSlice* r) {
    return guarded([&] {
        DevCtx d(k);
        need_text_order(k, pc);
        need(!next_count || count_alloc >= d.tiles, "next_count holds a tile each");
        for (u64 t = 0; t < d.tiles; t++) need((u64)tile_off[t] + 4096 <= alloc, "tile_off + 4096 beyond the lists");
        DevRun dr(r, d.tiles);
        Dev<u32> to(tile_off, d.tiles), nc(next_count, next_count ? count_alloc : 0);
        Dev<u64> dk(keys, alloc), dp(pos, alloc);
        gk::batch_fill(d.c, pc, bin_lo, bin_hi, to.p(), dk.p(), dp.p(), next_lo, next_hi, next_count ? nc.p() : nullptr, stream(), dr.rs);
        dk.down(keys); dp.down(pos); nc.down(next_count);
    });
}
KP int kp_gk_stage_fill(const KpCtx* k, int pc, u32 bin_lo, u32 bin_hi, const u32* tile_off, u32* staged, u32 alloc, u32 next_lo, u32 next_hi,
                        u32* next_count, u32 count_alloc) {
    return guarded([&] {
        DevCtx d(k);
        need_text_order(k, pc);
        need(!next_count || count_alloc >= d.tiles, "next_count holds a tile each");
        for (u64 t = 0; t < d.tiles; t++) need((u64)tile_off[t] + 4096 <= alloc, "tile_off + 4096 beyond the lists");
        Dev<u32> to(tile_off, d.tiles), nc(next_count, next_count ? count_alloc : 0), st(staged, alloc);
        gk::stage_fill(d.c, pc, bin_lo, bin_hi, to.p(), st.p(), next_lo, next_hi, next_count ? nc.p() : nullptr, stream());
        st.down(staged); nc.down(next_count);
    });
}
// staged: n entries; tile_off: a tile each; blk_tile, block_off: a block of 4096 entries each (blk_tile one more);
// keys, pos (alloc entries), next_count (count_alloc entries, or null): in/out
KP int kp_gk_stage_take(const KpCtx* k, const u32* staged, u64 n, u32 b0, u32 b1, const u32* block_off, u64* keys, u64* pos, u32 alloc,
                        u32 nb0, u32 nb1, u32* next_count, u32 count_alloc, const u32* tile_off, const u32* blk_tile) {
    return guarded([&] {
        DevCtx d(k);
        need(!k->skip && n < (1ull << 32), "text suffixes; a list below 2^32 entries");
        const u64 blocks = (n + 4095) / 4096;
        need(!next_count || count_alloc >= blocks, "next_count holds a block each");
        for (u64 b = 0; b < blocks; b++) need((u64)block_off[b] + 4096 <= alloc, "block_off + 4096 beyond the lists");
        for (u64 b = 0; b <= blocks && n; b++) need(blk_tile[b] < d.tiles && (b == 0 || blk_tile[b] >= blk_tile[b - 1]), "blk_tile ascends below the number of tiles");
        for (u64 t = 1; t < d.tiles; t++) need(tile_off[t] >= tile_off[t - 1], "tile_off ascends");
        for (u64 i = 0; i < n; i++) {           // the text position an entry names: its tile is the last whose offset is at most i
            const u64 t = (u64)(std::upper_bound(tile_off, tile_off + d.tiles, (u32)i) - tile_off);
            need(t >= 1 && (t - 1) * 4096 + (staged[i] & 4095u) < k->n, "a staged entry beyond the text");
            need(blk_tile[i >> 12] <= t - 1 && t - 1 <= blk_tile[(i >> 12) + 1], "blk_tile: a block's tiles lie between its entry and the next");
        }
        Dev<u32> st(staged, n), bo(block_off, blocks), nc(next_count, next_count ? count_alloc : 0), to(tile_off, d.tiles), bt(blk_tile, blocks + 1);
        Dev<u64> dk(keys, alloc), dp(pos, alloc);
        gk::stage_take(d.c, st.p(), n, b0, b1, bo.p(), dk.p(), dp.p(), nb0, nb1, next_count ? nc.p() : nullptr, to.p(), bt.p(), stream());
        dk.down(keys); dp.down(pos); nc.down(next_count);
    });
}
// pstart: n_phrases entries; keys, pos (alloc entries): in/out
KP int kp_gk_phrase_items(const KpCtx* k, const void* pstart, int wide, u32 n_phrases, const u32* rep, u32 D, u64* keys, u64* pos, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= D, "keys / pos hold D entries");
        for (u32 i = 0; i < D; i++) need(rep[i] < n_phrases && pos_at(pstart, wide != 0, rep[i]) <= k->n, "rep beyond the phrases, or a phrase start beyond the text");
        DevPos ps(pstart, n_phrases, wide != 0);
        Dev<u32> r(rep, D);
        Dev<u64> dk(keys, alloc), dp(pos, alloc);
        gk::phrase_items(d.c, ps.p(), wide != 0, r.p(), D, dk.p(), dp.p(), stream());
        dk.down(keys); dp.down(pos);
    });
}

// ---- rounds and results that read the context ------------------------------------------------------------------------------
// the entry of the giant dictionary an element at V index q would be given at `off`: the index must lie inside g_isa
static void check_giant_entry(const DevCtx& d, const KpCtx* k, u64 rec, u64 off) {
    if (!k->g_n) return;
    const u64 q = rec & ((1ull << k->pos_bits) - 1);
    if (off >= d.len_of(k, rec)) return;       // (only where alpha goes on at `off`: the kernels ask for no entry behind a spent alpha)
    const u32 ph = d.rank1(q + k->skip + k->w - 2);
    const u32 word = k->g_bits[ph >> 5];
    if (!((word >> (ph & 31)) & 1u)) return;
    const u32 lo = k->g_rank[ph >> 5] + (u32)__builtin_popcount(word & ((1u << (ph & 31)) - 1u));
    need(lo < k->g_n && k->g_k[lo] == ph, "g_bits / g_rank / g_k name the same giant occurrences");
    need(q + off >= k->g_ps[lo] && (u64)k->g_base[lo] + (q + off - k->g_ps[lo]) < k->n_gisa, "an element's giant entry beyond g_isa");
}
// keys (alloc entries), err (16 words): in/out; gr, pure, ghead: m entries each, or all null
KP int kp_gk_round_keys(const KpCtx* k, const u64* pos, u32 m, u64 offset, u64* keys, u32 alloc, u32* err, const u32* gr, const u8* pure,
                        const u32* ghead) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= m && ((gr && pure && ghead) || (!gr && !pure && !ghead)), "keys holds m entries; gr, pure and ghead together");
        d.check_elements(k, pos, m);
        for (u32 e = 0; e < m; e++) {
            need(!ghead || ghead[e] < m, "ghead beyond the list");
            check_giant_entry(d, k, pos[e], offset);
        }
        need(offset <= k->n + 64, "offset within the text");
        Dev<u64> p(pos, m), dk(keys, alloc);
        Dev<u32> e(err, 16), g(gr, gr ? m : 0), gh(ghead, ghead ? m : 0);
        Dev<u8> pu(pure, pure ? m : 0);
        gk::round_keys(d.c, p.p(), m, offset, dk.p(), e.p(), stream(), gr ? g.p() : nullptr, pure ? pu.p() : nullptr, ghead ? gh.p() : nullptr);
        dk.down(keys); e.down(err);
    });
}
// gr, pure (alloc entries): in/out
KP int kp_gk_giant_probe(const KpCtx* k, const u64* pos, const u32* ghead, u32 m, u64 offset, u32* gr, u8* pure, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= m, "gr / pure hold m entries");
        d.check_elements(k, pos, m);
        for (u32 e = 0; e < m; e++) { need(ghead[e] < m, "ghead beyond the list"); check_giant_entry(d, k, pos[e], offset); }
        Dev<u64> p(pos, m);
        Dev<u32> gh(ghead, m), g(gr, alloc);
        Dev<u8> pu(pure, alloc);
        gk::giant_probe(d.c, p.p(), gh.p(), m, offset, g.p(), pu.p(), stream());
        g.down(gr); pu.down(pure);
    });
}
// headval (alloc entries), err (16 words), lcp_out (lcp_alloc entries, or null; then slot is null too): in/out
KP int kp_gk_round_heads(const KpCtx* k, const u64* keys, const u32* ghead, u32 m, u32* headval, u32 alloc, u32* err, u32* lcp_out,
                         u32 lcp_alloc, const u32* slot, u64 offset, const u8* pure) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= m && (!lcp_out) == (!slot), "headval holds m entries; lcp_out and slot together");
        check_gheads(ghead, m);
        const bool giant_round = k->g_n != 0 && offset >= k->g_depth;
        for (u32 c = 0; c < m; c++) {
            need(!slot || slot[c] < lcp_alloc, "slot beyond lcp_out");
            const bool as_giant = (giant_round || (pure && pure[ghead[c]])) && (keys[c] >> 32) == (gk::GIANT_KEY >> 32);
            need(!as_giant || (k->g_n && (u32)keys[c] < k->n_gisa), "a giant key beyond the giant dictionary");
            // two entries of different groups inside one old group: ascending, as the round's sort leaves them (the range minimum
            // between them is asked for)
            if (as_giant && c > 0 && ghead[c] != c && (keys[c - 1] >> 32) == (gk::GIANT_KEY >> 32) && (u32)keys[c - 1] < k->n_gisa &&
                k->g_grp[(u32)keys[c]] != k->g_grp[(u32)keys[c - 1]])
                need((u32)keys[c - 1] < (u32)keys[c], "giant entries of one group ascend");
        }
        Dev<u64> dk(keys, m);
        Dev<u32> gh(ghead, m), hv(headval, alloc), e(err, 16), l(lcp_out, lcp_out ? lcp_alloc : 0), sl(slot, slot ? m : 0);
        Dev<u8> pu(pure, pure ? m : 0);
        gk::round_heads(d.c, dk.p(), gh.p(), m, hv.p(), e.p(), stream(), lcp_out ? l.p() : nullptr, slot ? sl.p() : nullptr, offset,
                        pure ? pu.p() : nullptr);
        hv.down(headval); e.down(err); l.down(lcp_out);
    });
}
// sa_lo (alloc entries), sa_hi (alloc bytes, or null: a 32-bit column), bwt (alloc bytes): in/out
KP int kp_gk_write_columns(const KpCtx* k, const u64* pos, u32 B, u64 base, u32* sa_lo, u8* sa_hi, u8* bwt, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        need(base + B <= alloc && !k->skip, "the columns hold base + B entries; text suffixes");
        d.check_elements(k, pos, B);
        Dev<u64> p(pos, B);
        Dev<u32> lo(sa_lo, alloc);
        Dev<u8> hi(sa_hi, sa_hi ? alloc : 0), bw(bwt, alloc);
        SaCol col; col.lo = lo.p(); col.hi = sa_hi ? hi.p() : nullptr;
        gk::write_columns(d.c, p.p(), B, base, col, bw.p(), stream());
        lo.down(sa_lo); hi.down(sa_hi); bw.down(bwt);
    });
}
// pid: the context's (m entries); prank (alloc entries): in/out
KP int kp_gk_phrase_ranks(const KpCtx* k, const u64* pos, u32 D, const u32* pid, u32* prank, u32 alloc) {
    return guarded([&] {
        DevCtx d(k);
        d.check_elements(k, pos, D);
        for (u32 j = 0; j < D; j++) need(pid[d.rank1((pos[j] & ((1ull << k->pos_bits) - 1)) + k->skip + k->w - 2)] < alloc, "pid beyond prank");
        Dev<u64> p(pos, D);
        Dev<u32> pi(pid, k->m), pr(prank, alloc);
        gk::phrase_ranks(d.c, p.p(), D, pi.p(), pr.p(), stream());
        pr.down(prank);
    });
}
// tab: n_tab records of four words; the seven columns (alloc entries), err (16 words): in/out
KP int kp_gk_expand_entries(const KpCtx* k, const u64* pos, const u32* lcp, u32 B, const u32* tab, u32 n_tab, u32* ce_cnt, u32* ce_first,
                            u32* ce_offm1, u8* ce_bwt, u32* ce_gs, u32* ce_hl, u32* ce_slen, u32 alloc, u32* err) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= B && k->pid && !k->skip, "the columns hold B entries; the context names pid; text suffixes");
        d.check_elements(k, pos, B);
        for (u32 e = 0; e < B; e++) need(k->pid[d.rank1((pos[e] & ((1ull << k->pos_bits) - 1)) + k->skip + k->w - 2)] < n_tab, "pid beyond tab");
        Dev<u64> p(pos, B);
        Dev<u32> l(lcp, B), tb(tab, 4 * (size_t)n_tab), c0(ce_cnt, alloc), c1(ce_first, alloc), c2(ce_offm1, alloc), c4(ce_gs, alloc),
            c5(ce_hl, alloc), c6(ce_slen, alloc), e(err, 16);
        Dev<u8> c3(ce_bwt, alloc);
        gk::expand_entries(d.c, p.p(), l.p(), B, tb.p(), c0.p(), c1.p(), c2.p(), c3.p(), c4.p(), c5.p(), c6.p(), e.p(), stream());
        c0.down(ce_cnt); c1.down(ce_first); c2.down(ce_offm1); c3.down(ce_bwt); c4.down(ce_gs); c5.down(ce_hl); c6.down(ce_slen); e.down(err);
    });
}

// out (out_alloc entries), flags (alloc entries), err (16 words), lcp_out (out_alloc entries, or null): in/out
KP int kp_gk_resolve_small(const KpCtx* k, const u64* pos, const u32* ghead, const u32* slot, u32 m, u64 offset, u64* out, u32 out_alloc,
                           u8* flags, u32 alloc, u32* err, u32* lcp_out, u32 limit) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= m, "flags holds m entries");
        check_gheads(ghead, m);
        d.check_compared(k, pos, m, offset);
        for (u32 e = 0; e < m; e++)                          // a group's slots are consecutive from its first member's
            need((u64)slot[ghead[e]] + (e - ghead[e]) < out_alloc, "a group's slots beyond out");
        Dev<u64> p(pos, m), o(out, out_alloc);
        Dev<u32> gh(ghead, m), sl(slot, m), e(err, 16), l(lcp_out, lcp_out ? out_alloc : 0);
        Dev<u8> f(flags, alloc);
        gk::resolve_small(d.c, p.p(), gh.p(), sl.p(), m, offset, o.p(), f.p(), e.p(), stream(), lcp_out ? l.p() : nullptr, limit);
        o.down(out); f.down(flags); e.down(err); l.down(lcp_out);
    });
}
// sl: the parse's LCP values (n_sl entries: the range-minimum view is built over them); carry: one record, or null;
// lcp (alloc entries), err (16 words): in/out
KP int kp_gk_batch_lcp(const KpCtx* k, const u32* sl, u32 n_sl, const u64* pos, u32 B, const u64* carry, u32* lcp, u32 alloc, u32* err) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= B && n_sl >= 1, "lcp holds B entries; sl at least one");
        d.check_compared(k, pos, B, 0);
        if (carry) d.check_compared(k, carry, 1, 0);
        for (u32 j = 0; j < B && !k->expand; j++) need(d.rank_key(k, pos[j]) < n_sl, "a parse rank beyond sl");
        need(!carry || k->expand || d.rank_key(k, carry[0]) < n_sl, "a parse rank beyond sl");
        Dev<u64> p(pos, B), cy(carry, carry ? 1 : 0);
        Dev<u32> v(sl, n_sl), l(lcp, alloc), e(err, 16);
        DevBuf<u32> bmin;
        RmqView R;
        R.sl = v.p(); R.m = n_sl;
        u32 levels = 0;
        build_rmq(v.p(), n_sl, bmin, R.nb, levels, stream());
        R.bmin = bmin.get();
        gk::batch_lcp(d.c, R, p.p(), B, carry ? cy.p() : nullptr, carry != nullptr, l.p(), e.p(), stream());
        l.down(lcp); e.down(err);
    });
}

// list: 4 regions of cap (first, size) pairs, n_groups[cl] of them used; sl: the parse's LCP values (n_sl entries);
// out (out_alloc entries), flags (alloc entries), lcp_out (out_alloc entries, or null), err (16 words): in/out
KP int kp_gk_resolve_medium(const KpCtx* k, const u32* sl, u32 n_sl, const u64* pos, u32 m, const u32* slot, const u32* list, u32 cap,
                            const u32* n_groups, u64 offset, u64* out, u32 out_alloc, u8* flags, u32 alloc, u32* lcp_out, u32* err) {
    return guarded([&] {
        DevCtx d(k);
        need(alloc >= m && n_sl >= 1, "flags holds m entries; sl at least one");
        d.check_compared(k, pos, m, offset);
        for (u32 e = 0; e < m && !k->expand && !k->skip; e++) need(d.rank_key(k, pos[e]) < n_sl, "a parse rank beyond sl");
        static const u32 seg[4] = {16, 32, 64, 128};
        for (u32 cl = 0; cl < 4; cl++) {
            need(n_groups[cl] <= cap, "a class has more groups than a region holds");
            for (u32 g = 0; g < n_groups[cl]; g++) {
                const u32 first = list[2 * ((size_t)cl * cap + g)], size = list[2 * ((size_t)cl * cap + g) + 1];
                need(size >= 1 && size <= seg[cl] && (u64)first + size <= m, "a listed group inside the list, not larger than its class");
                need((u64)slot[first] + size <= out_alloc, "a group's slots beyond out");
            }
        }
        Dev<u64> p(pos, m), o(out, out_alloc);
        Dev<u32> v(sl, n_sl), s2(slot, m), li(list, 8 * (size_t)cap), e(err, 16), l(lcp_out, lcp_out ? out_alloc : 0);
        Dev<u8> f(flags, alloc);
        DevBuf<u32> bmin;
        RmqView R;
        R.sl = v.p(); R.m = n_sl;
        u32 levels = 0;
        build_rmq(v.p(), n_sl, bmin, R.nb, levels, stream());
        R.bmin = bmin.get();
        gk::resolve_medium(d.c, R, p.p(), s2.p(), li.p(), cap, n_groups, offset, o.p(), f.p(), lcp_out ? l.p() : nullptr, e.p(), stream());
        o.down(out); f.down(flags); l.down(lcp_out); e.down(err);
    });
}
