/* mumemto_gpu.h -- device-resident entry points of libmumemto (MI355X).
 *
 * The drop-in ABI (mumemto.h) takes host strings, like the reference.  These
 * entry points expose the same hot path with inputs already in HBM, stage by
 * stage, for bench.py, the parity tests and multi-GPU drivers.  Plain C ABI:
 * pointers and sizes only.  Every call returns 0 on success; on failure the
 * message is in mmt_last_error() (thread-local) and nothing falls back to a
 * CPU path.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   text layout           RefBuilder::build_input_file   src/ref_builder.cpp:211-314, :330-384
 *   SA/LCP/BWT stream     gsacak_lcp / pfp_lcp::process  include/direct_gsacak.hpp:50-116,
 *                                                        include/pfp_lcp_mum.hpp:115-231
 *   match scan            mem_finder::update             include/mem_finder.hpp:161-170, :304-355
 *   writers               write_mum / write_mem / close  include/mem_finder.hpp:104-158, :210-263, :357-428
 *   partition merge       merge_partitions               src/merge_candidates.cpp:97-157
 */
#ifndef MUMEMTO_GPU_H
#define MUMEMTO_GPU_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__) || defined(__clang__)
#define MMT_API __attribute__((visibility("default")))
#else
#define MMT_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmt_engine mmt_engine;

/* Scan predicates, named as in mem_finder's constructor (mem_finder.hpp:53).
 * CLI flag normalisation (pfp_mum.hpp:149-198) is the caller's job.          */
typedef struct mmt_params {
    uint32_t min_match_len;   /* -l, default 20                               */
    uint64_t num_distinct;    /* matches must occur in >= this many docs; 0 = all */
    int64_t  max_doc_freq;    /* 1 = multi-MUM mode; 0 = unlimited            */
    int64_t  max_total_freq;  /* 0 = no cap                                   */
    uint8_t  use_revcomp;     /* text holds F$ R$ per document                */
    uint8_t  merge_metadata;  /* record candidate thresholds (-M / -n)        */
} mmt_params;

MMT_API const char* mmt_last_error(void);

/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or
 * NULL for a stream owned by the engine.                                      */
MMT_API int  mmt_engine_create(int device, void* hip_stream, mmt_engine** out);
MMT_API void mmt_engine_destroy(mmt_engine* e);

/* Input = concatenated raw forward bases of all documents (records of one
 * document concatenated, no separators; any case) + per-document lengths.
 * _device: d_bases is HBM memory borrowed until the next set_input/destroy.   */
MMT_API int mmt_engine_set_input_device(mmt_engine* e, const uint8_t* d_bases,
                                        const uint64_t* doc_len, size_t n_docs);
MMT_API int mmt_engine_set_input_host(mmt_engine* e, const uint8_t* h_bases,
                                      const uint64_t* doc_len, size_t n_docs);

/* Producer of the SA/LCP/BWT stream for the next runs:
 *   0 automatic | 1 direct suffix sort of the whole text (the reference's -g path, direct_gsacak.hpp)
 *   2 prefix-free parsing (the reference's default: newscan.hpp + pfp.hpp + pfp_lcp_mum.hpp)
 *   3 prefix-free parsing without the suffix array of the dictionary (guided.cpp: the text suffixes are sorted by their
 *     characters up to the phrase end, then by the parse; what 0 / 2 fall back to when the dictionary -- as large as
 *     half the text for two unrelated strands -- would not fit);
 *   4 the same with expansion: only one representative per (distinct phrase, offset) is sorted -- the valid suffixes of
 *     the dictionary -- and the emitter of 2 expands each by the inverted list of its phrase (pfp_lcp_mum.hpp:151-212);
 *     what 0 takes instead of 3 when the collection is redundant (a rank's share of whole genomes).
 *     mmt_producer_used reports 3 for both, mmt_producer_expanded says which;
 * w / p = PFP window and modulus (0 = chosen by the size of the text, as for the automatic producer; the reference's
 * defaults are 10 / 100).  The stream does not depend on them. */
MMT_API int mmt_engine_set_producer(mmt_engine* e, int kind, uint32_t w, uint32_t p);
/* Version of this device-resident ABI (the drop-in ABI of mumemto.h never changes).  Changes under an unchanged symbol name
 * bump it: 4 = mmt_merged_device hands out the 32-bit merged thresholds (uint16_t before) and mmt_partition gained
 * thresh_bits in former padding; 5 = producer 4 (expansion), mmt_producer_expanded, mmt_engine_set_text_sink keeps rows on
 * request.  A caller built against an older header checks this before it trusts the layout.                            */
MMT_API int mmt_abi_version(void);
MMT_API int mmt_producer_used(const mmt_engine* e);
MMT_API int mmt_producer_expanded(const mmt_engine* e);
/* Of the last run through the bucket-wise producer: out[0] = slices that bins of one repeated symbol (assembly gaps) were
 * produced in, out[1] = passes over the text that collected suffixes, out[2] = batches, out[3] = 1 when several batches
 * shared a pass (staging list).  Zeros for the other producers.                                                          */
MMT_API int mmt_producer_stats(const mmt_engine* e, uint64_t out[4]);

/* The row tap (test instrument of full-size runs that keep nothing else: tests/bigchecks.py check_bins_complete): every
 * accepted interval of the NEXT runs whose match begins with one of the n k-mers (n x k bytes, k <= 16) leaves a copy of its
 * length and of ALL its suffix-array entries (text positions) before its window drops it; n = 0 switches it off.
 * mmt_row_tap_counts: out[0] rows, out[1] entries tapped by the last run; mmt_row_tap_get: length[rows], occ_start[rows + 1],
 * sa[entries] (rows in no particular order; rc 3 when the capacities given here were exceeded).
 * mmt_kmer_positions: every position of the resident text whose suffix begins with one of the k-mers, ascending, with the
 * index of its k-mer; *found may exceed cap (only cap were written).  Together they give precision AND recall inside whole
 * bins of leading characters: the host sorts those suffixes, runs the oracle's scan over them and compares.                */
/* (bytes, digest) of what the last run's text sink wrote, in file order -- kept when the sink's path is "/dev/null" (the bytes
 * are formatted, copied out, digested and dropped: a full-size test run whose rows nobody can keep) or MMT_SINK_DIGEST is set */
MMT_API int mmt_text_sink_digest(const mmt_engine* e, uint64_t out[2]);
/* 1 when the suffixes that begin with this k-mer belong to the share of the stream the last run of the bucket-wise producer
 * produced (mmt_engine_set_scan_shard: whole bins of leading characters), 0 when not, -1 when that producer did not run */
MMT_API int mmt_kmer_in_share(const mmt_engine* e, const uint8_t* kmer, size_t k);
MMT_API int mmt_engine_set_row_tap(mmt_engine* e, const uint8_t* kmers, size_t n, size_t k, size_t max_rows, size_t max_occ);
MMT_API int mmt_row_tap_counts(mmt_engine* e, uint64_t out[2]);
MMT_API int mmt_row_tap_get(mmt_engine* e, uint32_t* length, uint64_t* occ_start, uint64_t* sa);
MMT_API int mmt_kmer_positions(mmt_engine* e, const uint8_t* kmers, size_t n, size_t k, uint64_t* pos, uint32_t* which,
                               uint64_t cap, uint64_t* found);

/* One pass of the hot path: text -> SA/LCP/BWT -> scan -> rows (+ thresholds). */
/* Stage checkpoints of the reference CLI (src/pfp_mum.cpp:97-111 `-a`, :122-124 `-p`): hand over the text T itself
 * (UPPER(F) '$' [revcomp(F) '$'] per document, n characters) or the stream of the real suffixes (sentinel entry
 * dropped; may be a prefix of the full stream).  mmt_engine_run then skips the stages that would have made them.  */
MMT_API int mmt_engine_set_text_host(mmt_engine* e, const uint8_t* text, uint64_t n, const uint64_t* doc_len,
                                     size_t n_docs, int use_revcomp);
MMT_API int mmt_engine_set_stream_host(mmt_engine* e, const uint32_t* sa, const uint32_t* lcp, const uint8_t* bwt,
                                       uint64_t entries, const uint64_t* doc_len, size_t n_docs, int use_revcomp);
MMT_API int mmt_engine_run(mmt_engine* e, const mmt_params* p);

/* The same job for host-resident input of any size.  When the text would exceed max_text_chars
 * (0 = the limit of one suffix array in this build, 2^32 - 4097 characters) the documents are
 * processed as partitions that share document 0 and merged like `anchor_merge` does
 * (README.md:124-141 of the reference); strict multi-MUMs only, byte-identical to a direct run.   */
MMT_API int mmt_engine_run_partitioned(mmt_engine* e, const uint8_t* h_bases, const uint64_t* doc_len,
                                       size_t n_docs, const mmt_params* p, uint64_t max_text_chars);
MMT_API size_t mmt_partitions_used(const mmt_engine* e);
/* The same job with the documents SUPPLIED one at a time instead of resident on the host: supplier(user, d, dst, doc_len[d])
 * writes the bases of document d to dst and returns 0 (non-zero aborts the run).  It is asked for the documents in order
 * (for all of them a second time if the text has to be rebuilt).  The reference streams its FASTA files through the parser
 * and never holds the collection (include/newscan.hpp:265-325); this entry is for collections that do not fit the host as
 * bytes either (BASELINE configs[4]: 287 GB of bases).  Always ONE text: no anchor partitions.                              */
typedef int (*mmt_doc_supplier)(void* user, uint64_t doc, uint8_t* dst, uint64_t len);
MMT_API int mmt_engine_run_supplied(mmt_engine* e, mmt_doc_supplier supplier, void* user, const uint64_t* doc_len,
                                    size_t n_docs, const mmt_params* p);
/* build_main in-process (src/pfp_mum.cpp:31-159): FASTA / FASTQ(.gz) files in (one document per file, read on all
 * host cores), PREFIX.mums | PREFIX.mems and PREFIX.lengths out (out_prefix NULL: nothing is written, the rows stay
 * available through the accessors below).  seconds (optional): [0] reading + parsing the files, [1] H2D + the whole
 * GPU path, [2] writing the outputs, [3] total.  mmt_params.merge_metadata is honoured as in mmt_engine_run.         */
MMT_API int mmt_engine_run_files(mmt_engine* e, const char* const* paths, size_t n_paths, const mmt_params* p,
                                 const char* out_prefix, uint64_t max_text_chars, double seconds[4]);
/* merged PREFIX.athresh (L_0 + 1 entries) after a partitioned run                                  */
MMT_API int mmt_copy_merged_thresh(const mmt_engine* e, uint16_t* out);

/* ---- results of the last run ------------------------------------------------
 * A run leaves its rows and the file bytes in HBM; each accessor below downloads what it
 * returns on first use (page-locked host memory owned by the engine, valid until the next run). */
MMT_API size_t mmt_num_rows(const mmt_engine* e);
MMT_API size_t mmt_num_docs(const mmt_engine* e);
/* MUM mode: length[n_rows], offsets[n_rows*n_docs] (-1 absent), strands (1 '+') */
MMT_API int mmt_rows_mum(const mmt_engine* e, uint32_t* length, int64_t* offsets, uint8_t* strands);
/* the same three tables where the run left them in HBM (valid until the next run): what a
 * multi-GPU exchange hands to RCCL without a host round trip                    */
MMT_API int mmt_rows_mum_device(const mmt_engine* e, const uint32_t** length, const int64_t** offsets,
                                const uint8_t** strands);
/* MEM mode: occ_start[n_rows+1]; flat offsets / doc ids / strands              */
MMT_API size_t mmt_num_occ(const mmt_engine* e);
MMT_API int mmt_rows_mem(const mmt_engine* e, uint32_t* length, uint64_t* occ_start,
                         int64_t* offsets, uint64_t* seq_ids, uint8_t* strands);
/* PREFIX.mums / PREFIX.mems bytes exactly as the CLI writes them.              */
MMT_API const char* mmt_output_text(mmt_engine* e, size_t* len);
/* PREFIX.bumbl bytes (MUM mode).                                               */
MMT_API const uint8_t* mmt_output_bumbl(mmt_engine* e, size_t* len);
/* candidate_thresh (u16, 2*(L_0+1) entries) when merge_metadata was set.       */
MMT_API size_t mmt_thresh_len(const mmt_engine* e);
MMT_API int mmt_copy_thresh(const mmt_engine* e, uint16_t* out);
/* Device pointers of the last run's thresholds / anchor ISA (for the merge).   */
MMT_API const uint16_t* mmt_thresh_device(const mmt_engine* e);
/* The engine's own threshold column: 32 bits per entry, never saturated (the 16-bit forms above are made from it and
 * saturate at 65535 like the reference's, include/mem_finder.hpp:299,328).  What partitions hand to the fold with
 * mmt_partition.thresh_bits = 32 and what the multi-GPU exchange carries. */
MMT_API int mmt_copy_thresh32(const mmt_engine* e, uint32_t* out);
MMT_API const uint32_t* mmt_thresh_device32(const mmt_engine* e);

/* ---- stage introspection (parity tests, bench roofline) ------------------- */
MMT_API uint64_t mmt_text_length(const mmt_engine* e);
MMT_API int mmt_copy_text(const mmt_engine* e, uint8_t* out);   /* n bytes    */
MMT_API int mmt_copy_sa(const mmt_engine* e, uint32_t* out);    /* n entries, real suffixes only */
MMT_API int mmt_copy_lcp(const mmt_engine* e, uint32_t* out);   /* lcp[0] = 0 */
MMT_API int mmt_copy_bwt(const mmt_engine* e, uint8_t* out);
/* Candidate lists of the last run, each entry {start, end, length, flags}
 * in real-suffix index space (= reference stream index - 1).                  */
MMT_API size_t mmt_num_candidates(const mmt_engine* e);
MMT_API int mmt_copy_candidates(const mmt_engine* e, uint32_t* out);
/* HIP-event times (ms) of the last run:
 * [0] text build  [1] suffix sort  [2] LCP+BWT  [3] scan kernel (roofline kernel)
 * [4] candidate verification + thresholds  [5] row gather + D2H  [6] the windows of the stream (emitter /
 * bucket batches; part of [1])  [7] whole run (host clock).                     */
MMT_API int mmt_stage_ms(const mmt_engine* e, float out[8]);
/* Bytes of the SA / LCP / BWT columns as stored (for the roofline model).     */
MMT_API int mmt_column_bytes(const mmt_engine* e, uint32_t out[3]);
/* Texts of 2^32 - 4096 characters or more run with 40-bit positions (the reference's width: include/common.hpp:59-60,
 * include/parse.hpp:45; dumps include/pfp_lcp_mum.hpp:323-369): the suffix-array column is stored as low word + high
 * byte, and the stream is scanned in ranges of suffix-array positions (mmt_scan_ranges of them in the last run).     */
MMT_API int mmt_is_wide(const mmt_engine* e);
/* the layout of the resident text (what mmt_merged_sequences reads): 1 = two bits per base and exception runs, 0 = a byte per base,
 * -1 = the engine holds no text                                                                                          */
MMT_API int mmt_engine_text_packed(const mmt_engine* e);
MMT_API size_t mmt_scan_ranges(const mmt_engine* e);
MMT_API int mmt_copy_sa64(const mmt_engine* e, uint64_t* out);    /* n entries, any text size */
/* mmt_engine_set_stream_host for streams with 40-bit suffix-array entries (sa_hi = bits 32..39)                        */
MMT_API int mmt_engine_set_stream_host40(mmt_engine* e, const uint32_t* sa_lo, const uint8_t* sa_hi, const uint32_t* lcp,
                                         const uint8_t* bwt, uint64_t entries, const uint64_t* doc_len, size_t n_docs,
                                         int use_revcomp);
/* Device heap of the engine's GPU (pool.hpp): [0] bytes mapped from the driver, [1] bytes in use, [2] high-water mark
 * of [1], [3] microseconds spent in the driver mapping memory.                                                         */
MMT_API int mmt_device_memory(const mmt_engine* e, uint64_t out[4]);
/* Multi-GPU runs of partial multi-MUMs / multi-MEMs, which the anchor merge cannot serve (the reference refuses to
 * merge them: include/pfp_mum.hpp:178-183): every rank builds the tables of the parse and then produces, scans and drops
 * ONLY ITS SHARE of the stream -- a range of suffix-array positions cut at multiples of 4096 (the parse proper), or whole
 * bins of leading characters (the bucket-wise producer: SURVEY.md 8(e), every reportable interval lies inside one bin).
 * No column is exchanged; the outputs of ranks 0 .. count-1, concatenated, are byte for byte the output of one GPU
 * (mmt_dist_gather_text, mumemto_amd/dist.py::run_sharded).  count = 1 switches it off.  mmt_sort_pieces: first entry and
 * number of entries of every rank's share (after a run).                                                              */
MMT_API int mmt_engine_set_scan_shard(mmt_engine* e, uint32_t index, uint32_t count);
MMT_API size_t mmt_sort_pieces(const mmt_engine* e, uint64_t* first, uint64_t* count, size_t capacity);
/* The columns of the stream exist one window at a time (the reference does not store them either:
 * include/pfp_lcp_mum.hpp:197).  on = 1: every window is also copied into whole columns, so that mmt_copy_sa / _lcp /
 * _bwt work after the run (tests, stage dumps); 0: never; -1 (default): for texts below 2^26 characters.               */
MMT_API int mmt_engine_keep_columns(mmt_engine* e, int on);
MMT_API int mmt_columns_kept(const mmt_engine* e);
/* Of the last run: [0] entries of the stream this engine produced (its share of a sharded run + the left extensions of its
 * windows), [1] bytes of the window buffers that held them (high-water mark: independent of the text length), [2] number
 * of windows, [3] bytes of the suffix-array entries that left the windows with accepted rows.                          */
MMT_API int mmt_stream_stats(const mmt_engine* e, uint64_t out[4]);
/* Returns the heap's physical memory to the driver when no engine buffer is live (long-lived hosts between jobs).  The engine
   the mumemto_library entry points (mumemto.h) share is let go first -- the next such call makes a new one --; engines made
   with mmt_engine_create are the caller's to destroy.                                                                      */
MMT_API void mmt_pool_trim(void);
/* bytes of device memory the heap leaves alone from now on (what MUMEMTO_HEAP_RESERVE sets for a whole process); ~0ull: back to
   the environment's value.  The estimates (automatic text limit, batch sizes, packing) see a device that much smaller. */
MMT_API void mmt_pool_set_reserve(unsigned long long bytes);
/* Text, window buffers and sort scratch of the last run go back to the device heap (downloaded results stay).
 * keep_anchor_ranks != 0: the suffix ranks of the anchor stay, so that mmt_merged_sort_like_direct still works -- the state
 * of a rank between its own pass and the fold of everybody's rows. */
MMT_API int mmt_engine_release_columns(mmt_engine* e, int keep_anchor_ranks);
/* PREFIX.mums / PREFIX.mems of the NEXT runs straight to `path` while a run goes on (NULL or "": off): the rows of a window of
 * the stream are final when it has been verified, so their bytes are formatted and written while the later windows are
 * produced (src/pfp_mum.cpp writes the file row by row as well, include/mem_finder.hpp:357-428).  A run over a text that
 * fills the device (packed text, or 2^37 characters and more; MMT_SINK_DISCARD=0/1 overrides) then keeps nothing of a
 * window's rows: it answers for the file and for mmt_num_rows only -- mmt_rows_* / mmt_output_text hold nothing. */
MMT_API int mmt_engine_set_text_sink(mmt_engine* e, const char* path);

/* ---- PFP stage checkpoints (the reference's -P / -K: PREFIX.dict, PREFIX.parse) ------------ */
/* Text layout + prefix-free parse only (newscan.hpp pfparser: process_string ... finish_parse).  */
MMT_API int mmt_engine_parse_only(mmt_engine* e, uint8_t use_revcomp, uint32_t w, uint32_t p);
/* out[0] #phrases of the parse, [1] #distinct phrases, [2] dictionary bytes, [3] #groups of equal
 * proper phrase suffixes, [4] doubling rounds on the dictionary, [5] on the parse, [6] #valid
 * dictionary suffixes, [7] #groups too large for an LDS tile (sorted by the segmented fallback)   */
MMT_API int mmt_pfp_counts(const mmt_engine* e, uint64_t out[8]);
/* dictionary suffixes of the last run that were ordered by the long run of one symbol they begin in (runs of assembly
   gaps, homopolymers: sorter.hpp, RunRefine) instead of by prefix doubling; -1: null engine */
MMT_API long long mmt_pfp_run_refined(const mmt_engine* e);
/* PREFIX.dict bytes (sorted phrases, 0x01 after each, 0x00 at the end; out holds counts[2] bytes)  */
MMT_API int mmt_pfp_copy_dict(mmt_engine* e, uint8_t* out);
/* PREFIX.parse entries (1-based phrase ranks, u32; out holds counts[0] entries)                    */
MMT_API int mmt_pfp_copy_parse(mmt_engine* e, uint32_t* out);
/* ms: [0] triggers+phrases [1] distinct phrases [2] dictionary text [3] dictionary SA
 * [4] dictionary LCP + groups + ranks [5] parse SA [6] text keys + sort [7] total (host clock)    */
MMT_API int mmt_pfp_stage_ms(const mmt_engine* e, float out[8]);

/* ---- anchor partition merge (src/merge_candidates.cpp:97-157) -------------- */
/* ZERO-INITIALISE this struct (`mmt_partition p = {0};` / `memset`): thresh_bits occupies what was padding before round 4,
 * and the merge entry points reject any value other than 0, 16 or 32 (rc 3).                                        */
typedef struct mmt_partition {
    uint64_t n_rows, n_docs;
    const uint32_t* length;   /* host or device (see rows_on_device)           */
    const int64_t*  offsets;  /* n_rows * n_docs, column 0 = anchor            */
    const uint8_t*  strands;  /* 1 = '+'                                       */
    const uint16_t* thresh;   /* host or device (see thresh_on_device), L_0+1 entries; uint32_t entries behind the same
                                 pointer when thresh_bits == 32 */
    uint64_t thresh_len;
    uint8_t thresh_on_device;
    uint8_t rows_on_device;   /* length / offsets / strands are HBM pointers   */
    uint8_t thresh_bits;      /* 0 or 16: the reference's PREFIX.athresh width (saturated at 65535, mem_finder.hpp:299);
                                 32: the engine's own width (mmt_copy_thresh32 / mmt_thresh_device32), never saturated --
                                 what the multi-GPU exchange carries */
} mmt_partition;
typedef struct mmt_merged mmt_merged;
/* Left fold over parts[0..k) exactly as anchor_merge does; the per-position
 * whole fold runs on the GPU of `e` and the merged rows stay in its HBM until
 * mmt_merged_get / mmt_merged_text copy them out.                              */
MMT_API int mmt_anchor_merge(mmt_engine* e, const mmt_partition* parts, size_t k, mmt_merged** out);
/* The same with the minimum length of a merged MUM stated.  The reference's tool hard-codes 20
 * (src/merge_candidates.cpp:141), which equals a direct run only for partitions made with -l 20: a multi-GPU run with
 * another -l passes that value here.                                                                                 */
MMT_API int mmt_anchor_merge_min_len(mmt_engine* e, const mmt_partition* parts, size_t k, uint32_t min_len,
                                     mmt_merged** out);
/* The same table computed as `slices` independent slices of the anchor: slice [lo, hi) folds from the rows
 * that start in [lo - margin, hi) and the thresholds of that range, margin = (k - 1) x the longest row + 1.  On one engine
 * the slices run one after the other; mmt_dist_merge_ranges gives every rank of a communicator its own.               */
MMT_API int mmt_anchor_merge_by_ranges(mmt_engine* e, const mmt_partition* parts, size_t k, int slices, uint32_t min_len,
                                       mmt_merged** out);
/* The arithmetic of that fold, on the host (no device needed): slice r of `world` is [bounds[0], bounds[1]) and folds from
 * [bounds[2], bounds[1]), for an anchor of thresh_len = L_0 + 1 entries, k partitions and a longest row of `longest`.    */
MMT_API int mmt_fold_slice_bounds(uint64_t thresh_len, int world, int r, size_t k, uint32_t longest, uint64_t bounds[3]);
MMT_API size_t mmt_merged_rows(const mmt_merged* m);
MMT_API size_t mmt_merged_docs(const mmt_merged* m);
MMT_API int mmt_merged_get(mmt_merged* m, uint32_t* length, int64_t* offsets, uint8_t* strands,
                           uint16_t* thresh);
/* the merged tables in HBM (owned by m); thresholds at the engine's width, 32 bits  */
MMT_API int mmt_merged_device(const mmt_merged* m, const uint32_t** length, const int64_t** offsets,
                              const uint8_t** strands, const uint32_t** thresh);
/* Rows folded elsewhere (a coordinate-range fold: every rank folds its slice of the anchor) as a merged
 * result of this engine: host arrays in, HBM tables out, so that mmt_merged_sort_like_direct / mmt_merged_text apply.  */
MMT_API int mmt_merged_from_rows(mmt_engine* e, const uint32_t* length, const int64_t* offsets, const uint8_t* strands,
                                 size_t n_rows, size_t n_docs, const uint16_t* thresh, size_t thresh_len,
                                 mmt_merged** out);
/* The device twin: row tables that already sit in the HBM of e's GPU (mmt_rows_mum_device of a direct run) become a merged
 * result without a round trip through the host; the tables are copied, so the result outlives the engine's next run.
 * It carries no thresholds.                                                                                            */
MMT_API int mmt_merged_from_rows_device(mmt_engine* e, const uint32_t* length, const int64_t* offsets,
                                        const uint8_t* strands, size_t n_rows, size_t n_docs, mmt_merged** out);
/* ---- collinear blocks (`mumemto collinear`: mumemto/collinear_block.py on mumemto/utils.py find_coll_blocks) ----------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * mmt_merged_collinear does on the device what the reference does between reading a .mums file and writing the sorted one:
 * rows with an absent document (-1) are dropped, the rest is put into ascending order of column 0 (stable), and every
 * maximal run of consecutive rows that are consecutive, in the direction of their strand, in EVERY column is a block
 * (first row, last row), first < last.  max_break > 0 also cuts a run between two rows whose gap in some column exceeds it
 * (0: no limit; the tool's default is 1000); min_singleton_length >= 0 makes every row outside all runs whose length is at
 * least that a block of its own (negative: none).  Blocks are numbered by their first row.  Equal starts within one column
 * are ordered by row, where the reference leaves the order to an unstable sort.  Fewer than 2^32 rows.
 * The blocks are attached to m and m's table becomes the filtered, sorted one: from here on mmt_merged_rows / _get / _device
 * / _text / _write_text answer for that table, and the text carries a fourth field, the block number or `-`.  Calling it
 * again recomputes the blocks; mmt_merged_sort_like_direct drops them.                                                   */
MMT_API int mmt_merged_collinear(mmt_engine* e, mmt_merged* m, uint32_t max_break, int64_t min_singleton_length,
                                 uint64_t* n_blocks);
/* lr receives 2 x n_blocks host entries: first row, last row of every block                                            */
MMT_API int mmt_merged_blocks(const mmt_merged* m, uint32_t* lr);
/* the same list in HBM, and the block of every row (0xFFFFFFFF: none); owned by m                                      */
MMT_API int mmt_merged_blocks_device(const mmt_merged* m, const uint32_t** lr, const uint32_t** row_block);
/* Of the last mmt_merged_collinear on m: out[0..4] HIP-event milliseconds of filter + sort of the table, column extraction,
 * column sorts, adjacency passes, blocks; [5] rows before, [6] rows kept, [7] columns that needed a sort, [8] columns found
 * ascending, [9] column batches, [10] 1 when the table itself was re-ordered, [11] blocks.                               */
MMT_API int mmt_merged_collinear_stats(const mmt_merged* m, double out[12]);
/* ---- inversion calls (`mumemto inversion`: mumemto/find_inversions.py find_reversals + inversion_coords) -----------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * They work on the state mmt_merged_collinear leaves on the device: n full rows in ascending order of column 0 and blocks
 * (first row, last row) in ascending order.  For every column i >= 1 the blocks are put into ascending order of the start of
 * their first row in i (equal starts by block number, where the reference leaves the order to an unstable sort); a run is a
 * maximal stretch of that order, at least two blocks, in which the block number falls by one from position to position.  A run
 * is a call when every block of it lies on '-' in column i (one '+' block discards the whole run), and the call is
 * (i, start, end, ref_start, ref_end): start = the start in i of the LAST row of the run's first block, end = the start in i
 * of the FIRST row of its last block plus that row's length, ref_start / ref_end the same two rows in column 0.  Calls are in
 * ascending order of (i, position of the run).  The tool runs mmt_merged_collinear(e, m, max_block_gap, -1, ...) first.
 *
 * mmt_merged_set_blocks attaches a block list read from a .bumbl file instead (lr: 2 x n_blocks host entries), the
 * reference's "pre-computed collinear blocks".  It refuses, rc 3 and a message: a block out of range, with first > last, or
 * blocks that are not ascending and disjoint; a table with a partial row; a table whose column 0 is not ascending.  The last
 * two depart from the reference, which would compute on -1 starts.  From here on the text carries the fourth field.       */
MMT_API int mmt_merged_set_blocks(mmt_engine* e, mmt_merged* m, const uint32_t* lr, uint64_t n_blocks);
/* max_length >= 0 keeps the calls with |end - start| <= max_length only (negative: no limit).  Fails with a message when m
 * carries no blocks.  Calling it again recomputes the calls; mmt_merged_collinear, mmt_merged_set_blocks and
 * mmt_merged_sort_like_direct drop them.                                                                                */
MMT_API int mmt_merged_inversions(mmt_engine* e, mmt_merged* m, int64_t max_length, uint64_t* n_calls);
/* out receives 5 x n_calls host entries: column, start, end, ref_start, ref_end of every call                          */
MMT_API int mmt_merged_inversion_calls(const mmt_merged* m, int64_t* out);
/* the same values in HBM; owned by m                                                                                   */
MMT_API int mmt_merged_inversion_calls_device(const mmt_merged* m, const int64_t** calls);
/* Of the last mmt_merged_inversions on m: out[0..2] HIP-event milliseconds of the gather of the block heads, column sorts,
 * run passes; [3] blocks, [4] columns that needed a sort, [5] columns skipped as ascending, [6] runs found before the strand
 * and length filters, [7] calls.                                                                                        */
MMT_API int mmt_merged_inversion_stats(const mmt_merged* m, double out[8]);
/* ---- coverage (`mumemto coverage`: mumemto/mum_coverage.py) -------------------------------------------------------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * What share of sequence c do the multi-MUMs of the table cover?  A row takes part in column c when its start there is not -1
 * and its length is at least min_length; its interval is [start, min(start + length, seq_lengths[c])): a row that starts at or
 * beyond the end of the sequence contributes nothing, one that runs over the end contributes up to it (the reference's slice
 * assignment into a bitmap of seq_lengths[c] bools).  covered[c] is the size of the union of those intervals; a run is a
 * maximal stretch of covered positions, half-open [begin, end), and intervals that touch belong to one run.  Strands play no
 * part.  Fewer than 2^32 rows, starts below 2^62.
 *
 * mmt_merged_coverage reads the table and changes nothing of it: rows, blocks and inversion calls of m stay as they are, and
 * partial rows are legal.  seq_lengths: n_docs host entries; seq_idx >= 0: that column, seq_idx == -1: every column (what the
 * reference needs one invocation and one pass over the file each for); covered (may be null) receives n_docs host entries,
 * 0 for a column not asked for.  It refuses, rc 3 and a message: a seq_idx outside [-1, n_docs), a null seq_lengths, a needed
 * seq_lengths[c] <= 0 (the reference divides by it).  A table without rows is legal: all 0, no runs.  Calling it again
 * replaces the results; mmt_merged_collinear and mmt_merged_sort_like_direct, which replace the table, drop them.          */
MMT_API int mmt_merged_coverage(mmt_engine* e, mmt_merged* m, const int64_t* seq_lengths, int64_t seq_idx,
                                int64_t min_length, uint64_t* covered);
/* run_begin receives n_docs + 1 host entries: the runs of column c are [run_begin[c], run_begin[c + 1]), none for a column not
 * asked for; runs receives 2 x run_begin[n_docs] host entries, begin and end of every run, ascending within a column.  runs
 * may be null, to ask for the sizes first.                                                                              */
MMT_API int mmt_merged_coverage_runs(const mmt_merged* m, uint64_t* run_begin, int64_t* runs);
/* the same two arrays in HBM; owned by m                                                                               */
MMT_API int mmt_merged_coverage_runs_device(const mmt_merged* m, const uint64_t** run_begin, const int64_t** runs);
/* Of the last mmt_merged_coverage on m: out[0..3] HIP-event milliseconds of the extraction, column sorts, running maximum +
 * sum, runs; [4] columns that needed a sort, [5] columns found ascending, [6] column batches, [7] runs in all.           */
MMT_API int mmt_merged_coverage_stats(const mmt_merged* m, double out[8]);
/* ---- MEM density (`mumemto/mem_density.py`) ---------------------------------------------------------------------------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * How many multi-MEM occurrences cover each position of each sequence, summed over bins of bin_width positions.  With
 * size = the maximum of seq_lengths, an occurrence (doc, start) of a row of length l adds 1 to the positions of doc that the
 * numpy slice start : start + l selects on an axis of `size` entries (the reference's `coverage[idx, start:start+l] += 1`):
 *   a = start < 0 ? max(start + size, 0) : min(start, size),  b = the same rule for start + l,  [a, b) when a < b, else nothing.
 * So the cut is at `size`, not at the sequence's own length, a negative start wraps as numpy wraps it (start -30, l 25 on
 * size 100 covers [70, 95); start -1, l 30 covers nothing), and strands play no part.  Bin k covers [k W, min((k + 1) W, size)),
 * nbins = ceil(size / W), and the result is the num x nbins table of the depths summed over each bin: exact 64-bit integers,
 * for W = 1 the reference's array.  A bin_width beyond size is taken as size (one bin per sequence).
 *
 * mmt_density_create makes the zeroed tables on e's device (24 x num x nbins bytes).  mmt_density_add_rows takes a host batch of
 * whole rows -- length[n_rows], occ_start[n_rows + 1] from 0, offsets and seq_ids[occ_start[n_rows]], the shape of mmt_rows_mem --
 * and may be called any number of times; mmt_density_add_engine adds the MEM rows of e's last run where they lie in HBM.
 * mmt_density_finish makes the table from everything added so far; adding after it goes on from what is there, so a caller can
 * read intermediate results (the accessors return rc 3 between an add and the next finish).  Every refusal is rc 3 and a message,
 * is decided before anything is launched and leaves the engine and the tables as they were: a null seq_lengths or null row
 * tables; num == 0; a length <= 0 (or beyond 2^40); bin_width == 0; tables that exceed what the device heap can give (the
 * message names the smallest bin width that fits); a seq_id >= num (the message names the first such row; the reference raises
 * IndexError); occ_start that does not begin at 0, is not ascending or ends beyond 2^40; mmt_density_add_engine after a
 * MUM-mode run, after a run whose text sink dropped the rows window by window, or with num different from the run's
 * documents.  A batch without rows or occurrences is legal.                                                                  */
typedef struct mmt_density mmt_density;
MMT_API int mmt_density_create(mmt_engine* e, const int64_t* seq_lengths, size_t num, uint64_t bin_width, mmt_density** out);
MMT_API void mmt_density_free(mmt_density* d);
MMT_API int mmt_density_add_rows(mmt_density* d, const uint32_t* length, const uint64_t* occ_start, const int64_t* offsets,
                                 const uint64_t* seq_ids, size_t n_rows);
MMT_API int mmt_density_add_engine(mmt_density* d, mmt_engine* e);
MMT_API int mmt_density_finish(mmt_density* d);
/* out[0] num, [1] nbins, [2] size, [3] the bin width in use                                                                */
MMT_API int mmt_density_shape(const mmt_density* d, uint64_t out[4]);
/* bins receives num x nbins host entries, row-major                                                                       */
MMT_API int mmt_density_bins(const mmt_density* d, uint64_t* bins);
/* the same table in HBM; owned by d, rewritten by the next mmt_density_finish                                              */
MMT_API int mmt_density_bins_device(const mmt_density* d, const uint64_t** bins);
/* out[0] HIP-event milliseconds of every add pass so far, [1] of the last finish pass; counted over every add: [2]
 * occurrences, [3] occurrences with start + l beyond size (cut there), [4] occurrences that covered nothing, [5] occurrences
 * with a negative start; [6] nbins, [7] the bin width in use.                                                              */
MMT_API int mmt_density_stats(const mmt_density* d, double out[8]);
/* ---- BED intervals (`mumemto bed`: mumemto/mum_to_bed.py) -----------------------------------------------------------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * The collinear blocks and the long multi-MUMs of the table as `contig <TAB> start <TAB> end <TAB> name <TAB> strand` lines in
 * the coordinates of the contigs (FASTA records) of a sequence.  Records of column c, in ascending order of their first row:
 *   with blocks attached (mmt_merged_collinear, mmt_merged_set_blocks): one per block (first, last) and one per row in no
 *     block with length >= min_singleton_length;
 *   without: one per row with a start in c (not -1) and length >= min_singleton_length.
 * A block whose last row is on '+' in c is [start[first], start[last] + length[last]), another one [start[last], start[first] +
 * length[first]); a row is [start, start + length).  The strand is that of the last row.  name = the block's number, or
 * -1 - i for a row, i = its rank among the rows with a start in c (the row number itself when no row is partial).  With
 * ends_k = len_0 + ... + len_k over the contigs of c, the contig is the first k with ends_k > begin (a contig of length 0 is
 * never chosen), rel_start = begin - (ends_k - len_k), rel_end = rel_start + (end - begin): an interval that runs over the end
 * of its contig is not split.  A begin at or beyond the total gets the last contig and is counted (stats [5]).
 *
 * mmt_merged_bed reads the table and changes nothing of it: rows, blocks, inversion calls and coverage stay.  The contigs of
 * column c are entries [contig_begin[c], contig_begin[c + 1]) of contig_len and name_begin; contig_begin has n_docs + 1 host
 * entries, name_begin one entry per contig and one more: name g is names[name_begin[g] .. name_begin[g + 1]).  seq_idx >= 0:
 * that column, -1: every column; n_records (may be null) receives the number of records.  It refuses, rc 3 and a message: a
 * seq_idx outside [-1, n_docs), null tables, a needed column without contigs or of total length 0, a negative contig length
 * and a name with a tab or a newline in a needed column.  Fewer than 2^32 rows.  Calling it again replaces the results;
 * mmt_merged_collinear, mmt_merged_set_blocks and mmt_merged_sort_like_direct drop them.                                  */
MMT_API int mmt_merged_bed(mmt_engine* e, mmt_merged* m, const uint64_t* contig_begin, const int64_t* contig_len,
                           const uint64_t* name_begin, const char* names, int64_t seq_idx, int64_t min_singleton_length,
                           uint64_t* n_records);
/* record_begin receives n_docs + 1 host entries: the records of column c are [record_begin[c], record_begin[c + 1]), none for
 * a column not asked for; records receives 5 x record_begin[n_docs] host entries: contig (within the column), rel_start,
 * rel_end, name, strand (1 = '+').  records may be null, to ask for the sizes first.                                      */
MMT_API int mmt_merged_bed_records(const mmt_merged* m, uint64_t* record_begin, int64_t* records);
/* the same two arrays in HBM; owned by m                                                                               */
MMT_API int mmt_merged_bed_records_device(const mmt_merged* m, const uint64_t** record_begin, const int64_t** records);
/* The lines of column col of the last mmt_merged_bed, formatted on the device; the bytes live until the next call on m.
 * Null (and a message) when no records are attached or col is out of range.                                             */
MMT_API const char* mmt_merged_bed_text(mmt_merged* m, int64_t col, size_t* len);
/* The same bytes to PATH.tmp, renamed to PATH when complete (a path that is no regular file, such as /dev/stdout, is written
 * as it is).                                                                                                            */
MMT_API int mmt_merged_bed_write_text(mmt_merged* m, int64_t col, const char* path);
/* Of the last mmt_merged_bed on m: out[0..3] HIP-event milliseconds of select, gather, contig lookup and of the text written
 * since; [4] records, [5] records clamped to the last contig, [6] column batches, [7] text bytes written since.          */
MMT_API int mmt_merged_bed_stats(const mmt_merged* m, double out[8]);
/* ---- contig labels (`mumemto label`: mumemto/get_sequence_info.py) ----------------------------------------------------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * Every start of the table also as (contig, offset inside that contig), and the table as lines of six fields:
 *   LEN <TAB> s_0,...,s_{N-1} <TAB> +|-,... <TAB> BLOCK <TAB> c_0,...,c_{N-1} <TAB> rel_0,...,rel_{N-1}
 * one per row, in row order, nothing filtered.  With ends_k = len_0 + ... + len_k over the contigs of column c, cell (r, c) with
 * start s gets the first k with ends_k > s (a contig of length 0 is never chosen) and rel = s - (ends_k - len_k); an absent
 * cell (s == -1) gets contig 0 and rel -1, and is printed as -1 in fields 2 and 6.  BLOCK is * for a table without blocks, else
 * the number of the row's block among those attached when the text is asked for (mmt_merged_collinear, mmt_merged_set_blocks),
 * or -.  Field 5 holds the decimal contigs, or with use_names their names (the name of contig 0 for an absent cell).
 *
 * mmt_merged_label reads the table and changes nothing of it: rows, blocks, inversion calls, coverage and BED records stay;
 * partial rows and a table without rows (0 bytes) are legal.  The contig tables have the shape mmt_merged_bed takes, for every
 * column; name_begin and names are read with use_names only and may be null without.  text_bytes (may be null) receives the
 * length of the text.  It refuses, rc 3 and a message: null tables, a column without contigs or of total length 0, a negative
 * contig length, with use_names a name with a tab, a newline or a comma, and a start at or beyond the total of its sequence:
 * the message names the first such (row, column) in row-major order, its start and the total.  After a refused call no
 * labels are attached, those of an earlier call included.
 * Fewer than 2^32 rows.  Calling it again replaces the results; mmt_merged_collinear and mmt_merged_sort_like_direct drop
 * them, mmt_merged_set_blocks keeps them.  Before mmt_merged_label the accessors below return rc 3 (null for the text).   */
MMT_API int mmt_merged_label(mmt_engine* e, mmt_merged* m, const uint64_t* contig_begin, const int64_t* contig_len,
                             const uint64_t* name_begin, const char* names, int use_names, uint64_t* text_bytes);
/* contig and rel receive n_rows x n_docs host entries each, row-major like the table; either may be null              */
MMT_API int mmt_merged_label_cells(const mmt_merged* m, uint32_t* contig, int64_t* rel);
/* the same two arrays in HBM; owned by m                                                                               */
MMT_API int mmt_merged_label_cells_device(const mmt_merged* m, const uint32_t** contig, const int64_t** rel);
/* The lines of the last mmt_merged_label, formatted on the device; the bytes live until the next call on m.  Null (and a
 * message) when no labels are attached.                                                                                 */
MMT_API const char* mmt_merged_label_text(mmt_merged* m, size_t* len);
/* The same bytes, formatted and written in pieces of whole rows, to PATH.tmp, renamed to PATH when complete (a path that is no
 * regular file, such as /dev/stdout, is written as it is).                                                              */
MMT_API int mmt_merged_label_write_text(mmt_merged* m, const char* path);
/* Of the last mmt_merged_label on m and of the text asked for since: out[0..3] HIP-event milliseconds of the lookup, of measure
 * + prefix sum, of the write, and of the copies to the host + the wait for the file; [4] cells, [5] absent cells, [6] columns
 * whose contig ends were searched in HBM rather than LDS, [7] bytes of the text as last measured.                       */
MMT_API int mmt_merged_label_stats(const mmt_merged* m, double out[8]);
/* ---- multi-MUM sequences (`extract_mums`: src/extract_mums.cpp, mumemto/extract_mums.py) --------------------------------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * The bases of the rows of column col as a multi-FASTA, measured and formatted on the device.  Record i, i = the row's index
 * in table order, is `>mum_<i>\n`, the bases, `#` unless terminator is 0, and the record separator.  The two forms of the
 * reference are two dialects:
 *   mmt_seq_binary (src/extract_mums.cpp): bytes as they are; strands ignored, always the forward slice; every record ends in
 *     \n; a row without a start in col (-1) or with a start beyond the document's end is refused;
 *   mmt_seq_python (mumemto/extract_mums.py): bases upper-cased; rows on '-' reverse-complemented (A<->T, C<->G, M<->K, R<->Y,
 *     V<->B, H<->D, every other byte unchanged); records joined by \n, none behind the last; a row without a start or with a
 *     start beyond the end is an empty record.
 * In both a row that runs over the document's end is cut there and one that starts exactly at the end is an empty record.
 *
 * Three sources: mmt_merged_sequences reads the engine's own text after a run (one byte per base or packed; always upper
 * case), where the table's columns are the engine's documents; mmt_merged_sequences_host takes the n_bases bases of document
 * col from the host; mmt_merged_sequences_file reads them from a FASTA file, plain or gzip, records concatenated (n_bases,
 * may be null, receives their number).  text_bytes (may be null) receives the length of the text.
 * They read the table and change nothing of it: rows, blocks, inversion calls, coverage, BED records and labels stay; a table
 * without rows gives an empty text.  They refuse, rc 3 and a message: col outside [0, n_docs), a start below -1, 2^32 rows or
 * more, null bases with n_bases > 0, an unknown dialect, a resident source when the engine holds no text or has another number
 * of documents than the table has columns, and the dialect's refusals, naming the first such row.  After a refused call no
 * sequences are attached, those of an earlier call included.  Calling one again replaces the results; mmt_merged_collinear
 * and mmt_merged_sort_like_direct drop them.  Before them the accessors below return rc 3 (null for the text).            */
enum mmt_seq_dialect { mmt_seq_binary = 0, mmt_seq_python = 1 };
MMT_API int mmt_merged_sequences(mmt_engine* e, mmt_merged* m, int64_t col, int dialect, int terminator, uint64_t* text_bytes);
MMT_API int mmt_merged_sequences_host(mmt_engine* e, mmt_merged* m, const uint8_t* bases, uint64_t n_bases, int64_t col,
                                      int dialect, int terminator, uint64_t* text_bytes);
MMT_API int mmt_merged_sequences_file(mmt_engine* e, mmt_merged* m, const char* fasta_path, int64_t col, int dialect,
                                      int terminator, uint64_t* n_bases, uint64_t* text_bytes);
/* offsets receives n_rows + 1 host entries: record i is bytes [offsets[i], offsets[i + 1]) of the text                   */
MMT_API int mmt_merged_sequences_offsets(const mmt_merged* m, uint64_t* offsets);
/* the same array in HBM; owned by m                                                                                     */
MMT_API int mmt_merged_sequences_offsets_device(const mmt_merged* m, const uint64_t** offsets);
/* The text of the last mmt_merged_sequences*, formatted on the device; the bytes live until the next call on m.  Null (and a
 * message) when no sequences are attached, or when the engine has laid out a text again (a run, a text or a stream handed
 * over) since a resident call: the records are then measured anew.                                                       */
MMT_API const char* mmt_merged_sequences_text(mmt_merged* m, size_t* len);
/* The same bytes, formatted and written in pieces of whole records, to PATH.tmp, renamed to PATH when complete (a path that is
 * no regular file, such as /dev/stdout, is written as it is).                                                            */
MMT_API int mmt_merged_sequences_write_text(mmt_merged* m, const char* path);
/* Of the last mmt_merged_sequences* on m and of the text asked for since: out[0] HIP-event milliseconds of measure + prefix
 * sum, [1] of the format kernel; [2] records, [3] bases written, [4] rows cut at the document's end, [5] empty records,
 * [6] bytes of the text, [7] pieces formatted since.                                                                     */
MMT_API int mmt_merged_sequences_stats(const mmt_merged* m, double out[8]);
/* ---- string-based merge, last step (`mumemto merge` without a common anchor: mumemto/merge_mums.py:211-307) ------------------
 * Callers detect these entry points by their symbols; mmt_abi_version() did not change for them.
 * The partitions were run with -M (PREFIX.thresh / .thresh_rev), their MUM strings extracted as `#`-terminated records
 * (extract_mums) and the multi-MUMs of those collections found ("MUMs of MUMs", mom).  mmt_string_fold maps every row of mom
 * back through the partitions' rows and merges the threshold tables, on the device; the closed form is
 * mumemto_amd/merge_mums.py string_merge, and the results equal it byte for byte:
 *   - a row of mom is cut at the `#` of collection 0 it spans; a piece shorter than 20 is dropped unless it is the whole row;
 *   - in every partition i the piece lies in a record (the first whose end is beyond its start there); it survives when in every
 *     partition that record exists and 0 != thresh_i[start] < the piece's length (indices clamped into the table);
 *   - the row of a surviving piece has the columns of every partition in turn: the start of the record's row + the piece's
 *     distance from the record's left end on a `+` cell, from its right end on a `-` cell, and the cell's strand, flipped when
 *     the piece matched reversed in collection i; rows in ascending order of column 0, equal starts in the order of the pieces;
 *   - thresholds per position of a row: the maximum over the partitions when all are > 0, else 0 (thresh_i and thresh_rev_i
 *     change places for a partition whose piece matched reversed); one 0 follows every row.
 * All arrays below are host arrays.  records holds, for collection i, the record lengths [begin[i], begin[i + 1]) as mom's
 * .lengths file lists them (the last record of a collection is shorter than its row + 1: do not derive them from the rows).
 * It refuses, rc 3 and a message, before anything is launched over the table at fault: S that is not mom's n_docs or
 * records->n_collections ("input # of MUM files does not match merged MUM input file"); a table of 2^32 - 1 rows or more; 2^32 - 256
 * pieces or more; a partition without columns; a negative record length; more records in collection i than rows in partition i;
 * a start of -1 in a partition or in mom; a partition whose column 0 is not ascending; thresh_len that is not the sum of
 * length + 1 over the partition's rows.  The engine stays usable after a refusal.
 * *out is a merged result like any other (mmt_merged_get / _text / _write_text / _collinear ...; it carries no anchor
 * thresholds) that also holds the two merged tables until a call that replaces its table (mmt_merged_collinear,
 * mmt_merged_sort_like_direct).                                                                                          */
typedef struct mmt_string_part {
    uint64_t n_rows, n_docs;
    const uint32_t* length;     /* n_rows                                         */
    const int64_t*  starts;     /* n_rows * n_docs, rows in ascending order of column 0 */
    const uint8_t*  strands;    /* 1 = '+'                                        */
    const uint16_t* thresh;     /* thresh_len entries each; not read for mom      */
    const uint16_t* thresh_rev;
    uint64_t thresh_len;
} mmt_string_part;
typedef struct mmt_string_records {
    uint64_t n_collections;
    const uint64_t* begin;      /* n_collections + 1                              */
    const int64_t*  length;     /* begin[n_collections] record lengths (MUM length + 1 for the `#`) */
} mmt_string_records;
MMT_API int mmt_string_fold(mmt_engine* e, const mmt_string_part* parts, size_t S, const mmt_string_part* mom,
                            const mmt_string_records* mom_records, mmt_merged** out);
/* entries of either merged threshold table: the sum of length + 1 over the merged rows; 0 for a result of another kind   */
MMT_API uint64_t mmt_merged_string_thresh_len(const mmt_merged* m);
/* host copies of the two tables; either may be null.  rc 3 when m carries none.                                          */
MMT_API int mmt_merged_string_thresh(const mmt_merged* m, uint16_t* thresh, uint16_t* thresh_rev);
/* the same two tables in HBM; owned by m                                                                                */
MMT_API int mmt_merged_string_thresh_device(const mmt_merged* m, const uint16_t** thresh, const uint16_t** thresh_rev);
/* Of the mmt_string_fold that made m: out[0..3] HIP-event milliseconds of split, locate and test, assemble + sort + permute,
 * thresholds; [4] pieces the rows of mom were cut into, [5] pieces dropped as shorter than 20, [6] pieces dropped by a
 * partition's records or thresholds, [7] merged rows.                                                                    */
MMT_API int mmt_merged_string_fold_stats(const mmt_merged* m, double out[8]);
/* Re-order merged rows into the order of a direct run (lexicographic by match
 * string) using the anchor suffix ranks of the engine's last run, whose
 * document 0 must be the anchor.                              */
MMT_API int mmt_merged_sort_like_direct(mmt_engine* e, mmt_merged* m);
MMT_API const char* mmt_merged_text(mmt_merged* m, size_t* len);
/* PREFIX.mums straight from the library (no copy of the bytes through the caller) */
MMT_API int mmt_merged_write_text(mmt_merged* m, const char* path);
MMT_API void mmt_merged_free(mmt_merged* m);

/* ---- multi-GPU exchange, one process per GPU (RCCL over xGMI) ------------------------------
 * Replaces the files + second tool between partitions of the reference's workflow (README.md:124-141: PREFIX.mums and
 * PREFIX.athresh per partition, then `anchor_merge`, src/merge_candidates.cpp:170-255; Python side
 * mumemto/merge_mums.py:141-183).  Rank 0 makes a unique id and hands it to the other ranks out of band (a file, an
 * environment variable, MPI, torch's store); every call below is collective over the communicator.  RCCL is bound at run
 * time (a copy already in the process, else /opt/rocm/lib/librccl.so).                                              */
typedef struct mmt_comm mmt_comm;
MMT_API int  mmt_comm_unique_id(uint8_t id[128]);
MMT_API int  mmt_comm_create(mmt_engine* e, int rank, int world, const uint8_t id[128], mmt_comm** out);
MMT_API void mmt_comm_destroy(mmt_comm* c);
/* Strict multi-MUMs: e's last run = this rank's partition {anchor} + its documents with merge metadata on.  Row tables
 * and thresholds of ranks 1 .. world-1 travel HBM -> HBM to rank 0 (ncclSend / ncclRecv, one group), rank 0 folds them on its GPU and
 * re-sorts into direct-run order: *out is the merged result on rank 0 (mmt_merged_text / _get / _free) and NULL on the
 * other ranks.  min_len = the run's -l (the reference's tool hard-codes 20).                                          */
MMT_API int  mmt_dist_merge(mmt_comm* c, mmt_engine* e, uint32_t min_len, mmt_merged** out);
/* The same result with the fold itself spread over the ranks (dist.cpp dist_merge_ranges): rows are broadcast, of the
 * thresholds -- 2 bytes per anchor position and rank -- every rank receives only its slice of the anchor from every other
 * rank (all-to-all), folds it, and sends its piece to rank 0.  mmt_dist_merge does this by itself from four ranks on
 * (MUMEMTO_RANGE_FOLD=0 / 1 overrides).                                                                                */
MMT_API int  mmt_dist_merge_ranges(mmt_comm* c, mmt_engine* e, uint32_t min_len, mmt_merged** out);
/* Modes without a partition merge (mmt_engine_set_scan_shard): the ranks' output bytes, concatenated in rank order, on
 * rank 0 (*len = 0 elsewhere); valid until the next call on this communicator.                                        */
MMT_API int  mmt_dist_gather_text(mmt_comm* c, const char** text, size_t* len);
/* Self-test of the exchange's message machinery with this rank as its own peer (dist.cpp dist_loopback): the row tables and
 * the 32-bit threshold column of the engine's last run (merge metadata on) through ncclSend / ncclRecv in one group, in pieces
 * of at most 2^30 elements, an all-gather and a broadcast; out = bytes moved, pieces, largest piece (bytes), elements that
 * arrived different (0 is the answer), microseconds, rows, row cells, thresholds.                                         */
MMT_API int  mmt_comm_loopback(mmt_comm* c, uint64_t out[8]);
/* One message of `elements` elements of `width` bytes (1, 4, 8) to this rank itself through ncclSend / ncclRecv in the pieces the
 * exchange cuts (MUMEMTO_RCCL_CHUNK): out = elements that arrived different, pieces, largest piece (bytes), microseconds.      */
MMT_API int  mmt_comm_selftest(mmt_comm* c, uint64_t elements, uint32_t width, uint64_t out[4]);
/* Every message of mmt_dist_merge / _merge_ranges / _gather_text is verified: the sender digests each piece of
 * its send buffers and sends the digests behind the data in the same group (one ncclUint64 trailer per receiver), the receiver
 * digests what arrived and compares on its GPU before anything reads the data.  A mismatch on ANY rank makes the call fail on
 * EVERY rank (rc != 0; mmt_last_error names the detecting rank and, on that rank, peer, table, piece and bytes).
 * MUMEMTO_EXCHANGE_VERIFY=0 switches it off; rank 0's value decides for all ranks.
 * mmt_comm_verify_stats, counted since the communicator was created: out[0] messages digested (sent + received), [1] their
 * pieces, [2] their bytes, [3] pieces that arrived different, [4] microseconds in the digest kernels (HIP events), [5] peer,
 * [6] table (0 lengths, 1 offsets, 2 strands, 3 thresholds, 4 text, 5 digests = the trailer itself) and [7] piece of the first
 * mismatch, all ones if there was none.                                                                                     */
MMT_API int  mmt_comm_verify_stats(mmt_comm* c, uint64_t out[8]);
/* The digest kernel by itself, for users with a transport of their own: `elements` elements of `width` bytes (1, 4, 8) at
 * device_ptr (aligned to width, current device), cut into pieces of piece_elements; out_host gets two words per piece -- sum
 * word, xor word -- for max(1, ceil(elements / piece_elements)) pieces.  For element i of a piece (0-based inside it) with
 * value v zero-extended to 64 bits, mod 2^64:  x = v + (i + 1) * 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;
 * x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;  sum += x;  xor ^= x.                                            */
MMT_API int  mmt_exchange_digest(const void* device_ptr, uint64_t elements, uint32_t width, uint64_t piece_elements,
                                 uint64_t* out_host);
/* The same on a copy of a host array in a fresh device allocation, starting skip_elements into it (a base that is not
 * 16-byte aligned); elements counts the whole array.                                                                        */
MMT_API int  mmt_exchange_digest_host(const void* host_ptr, uint64_t elements, uint32_t width, uint64_t skip_elements,
                                      uint64_t piece_elements, uint64_t* out_host);

#ifdef __cplusplus
}
#endif
#endif /* MUMEMTO_GPU_H */
