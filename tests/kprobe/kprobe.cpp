// kprobe.cpp -- test infrastructure: plain C entry points around single launch wrappers of the suffix sorter
// (mmt::k, mmt::prims, pk::pack_keys_u32, DoublingSorter::sort), for tests/kprobe.py.
//
// Every kp_* function takes host arrays, uploads them, calls exactly ONE wrapper, synchronises and copies the results
// back; arrays marked "in/out" go up as the caller filled them (sentinel patterns: what the wrapper must not touch
// comes back unchanged).  Errors: a non-zero return code, the message through kp_last_error() (as mmt_last_error).
// The library links the product's own objects (the classes are hidden symbols of libmumemto.so), so it carries its
// own copy of the device heap and of the switch table; nothing of the product is restated here.
//
// Adding a wrapper: one KP function below (upload with Dev<T>, call, down()), one ctypes line in tests/kprobe.py.
#include <cstdint>
#include <cstring>
#include <string>

#include <hip/hip_runtime.h>

#include "device_utils.hpp"
#include "kernels.hpp"
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
