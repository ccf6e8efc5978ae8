/*
 * classmate_hip.h — C ABI of libclassmate_hip.so, the MI355X (gfx950) hybrid
 * retrieval engine behind CLASSMATE-RAG's retrieval API.
 *
 * Plain C: pointers + sizes only, no C++/torch types.  Every entry point
 * names the reference interface it replaces (paths relative to the
 * taha-kms/CLASSMATE-RAG tree).  Conventions:
 *   - return 0 (CM_OK) on success, < 0 on error; cm_last_error() gives a
 *     thread-local message.  CM_EINVAL maps to Python ValueError (the
 *     reference's convention for length mismatches, e.g. bm25.py:152-153),
 *     CM_EZERODIV to ZeroDivisionError (rank_bm25 on an empty vocabulary,
 *     SURVEY.md §8a quirk Q7), everything else to RuntimeError.
 *   - "host" functions take caller-owned host arrays, run on the handle's
 *     own HIP stream and return after the results are copied back.
 *   - "_dev" functions take device pointers plus a hipStream_t (as void*;
 *     NULL = the null/default stream, which is torch's default stream too);
 *     they never allocate, never synchronise, and are safe to capture into a
 *     HIP graph.  Handles' private streams (host functions) are blocking, so
 *     they are ordered after work queued on the null stream.
 *   - rows are int64 row indices into the handle's storage; "-1" pads
 *     results that have fewer than k entries.
 *   - allow bitmaps: bit (r & 31) of word r >> 5 set => row r may be
 *     returned (a Chroma `where` / BM25 `_matches_filter` mask).
 */
#ifndef CLASSMATE_HIP_H
#define CLASSMATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CM_OK 0
#define CM_EINVAL (-1)
#define CM_ENOMEM (-2)
#define CM_EDEVICE (-3)
#define CM_EZERODIV (-4)
#define CM_EUNSUPPORTED (-5)

#define CM_DTYPE_F32 0
#define CM_DTYPE_BF16 1
#define CM_DTYPE_F16 2
#define CM_DTYPE_I32 3
#define CM_DTYPE_I64 4

/* Library ------------------------------------------------------------- */
const char *cm_last_error(void);
int cm_version(void);
int cm_device_count(int *n);
/* A HIP stream restricted to the CUs whose bits are set in cu_mask (n_words
 * 32-bit words; bit i = CU i of the device's enumeration) -- for running a
 * latency-bound stage beside a bandwidth-bound one (bench.py --bm25-cus).
 * Not a reference interface: an engine-side scheduling helper. */
int cm_stream_create_cu_masked(int device, const uint32_t *cu_mask, int n_words, void **out_stream);
int cm_stream_destroy(void *stream);
/* largest k the fused top-k kernels accept (dense and BM25 _dev entries); the
 * host-array searches accept any k >= 1 (beyond it: full order + device sort). */
int cm_max_topk(void);

/* Dense cosine k-NN ---------------------------------------------------
 * Replaces ChromaVectorStore (rag/retrieval/vector_chroma.py:81-278) and
 * the chromadb/hnswlib server it talks to: the corpus lives in HBM as fp32
 * rows, search is exact brute-force cosine (distance = 1 - cos, the
 * `hnsw:space=cosine` metric set at vector_chroma.py:156).               */
typedef struct cm_dense cm_dense;

/* ChromaVectorStore.__init__/_ensure_collection (vector_chroma.py:81-164). */
int cm_dense_create(int device, int32_t dim, int64_t capacity, cm_dense **out);
void cm_dense_destroy(cm_dense *h);
int cm_dense_reserve(cm_dense *h, int64_t capacity);
/* Device bytes of the row arrays (fp32 rows, norms, live bits, f16 plane): now and the most ever
 * held at once, and how many growths went through host memory (cm_dense_set_growth decides when).
 * Not a reference interface (capacity planning for 288 GB). */
int cm_dense_mem_stats(cm_dense *h, int64_t *cur_bytes, int64_t *peak_bytes, int64_t *staged_growths);
/* Growth policy (no reference counterpart: Chroma grows its own collection).  0 = automatic: a
 * growth copies device to device when the new arrays fit in the free device memory next to the old
 * ones, else it stages the rows through host memory; 1 = a store above 1 GiB always stages (peak
 * device footprint = the final allocation, never old + new).  CM_EINVAL for other modes. */
int cm_dense_set_growth(cm_dense *h, int32_t mode);
/* ChromaVectorStore.upsert (vector_chroma.py:168-200): write n fp32 rows
 * (host, n x dim row-major) at the given row indices, marking them live.
 * Rows beyond the current size grow the store. */
int cm_dense_upsert(cm_dense *h, const float *vecs, const int64_t *rows, int64_t n);
/* device variant: n contiguous rows starting at row0 from a device buffer. */
int cm_dense_upsert_dev(cm_dense *h, const float *vecs_dev, int64_t row0, int64_t n, void *stream);
/* col.delete (vector_chroma.py:181-187): clear the live bit of rows. */
int cm_dense_delete(cm_dense *h, const int64_t *rows, int64_t n);
/* vec_store.compact(), the hook vacuum_indexes probes for (rag/admin/backup.py:178-202): give the
 * rows that col.delete (rag/retrieval/vector_chroma.py:181-187) marked dead back.  The live rows of
 * [0, size) move to [0, n) in ascending order (ties -> lower row and the insertion order survive),
 * size becomes n, and everything at rows >= n is cleared as in a never-written store.
 * old_rows_out (nullable; caller-owned host memory for expect_live entries, or for
 * cm_dense_live_count entries when expect_live < 0) receives the old row of every new row;
 * *new_size (nullable) receives n.  expect_live >= 0 that differs from the device's live count ->
 * CM_EINVAL, a failed staging allocation -> CM_ENOMEM, both before anything is modified.  A store
 * without dead rows is left untouched (the map is the identity).  shrink != 0: also reallocate
 * the row arrays at round_up(max(n, 128), 128) rows when that is smaller (device to device when old
 * and new fit in free memory, else through the host; a store that fits neither way keeps its arrays,
 * which is not an error).  Host function: waits for the device's pending work, runs on the handle's
 * stream and returns when done; no search or upsert may run concurrently.  Under cm_dense_timing
 * a compaction that moves rows records three event pairs: rank, move, plane rebuild + tail. */
int cm_dense_compact(cm_dense *h, int64_t expect_live, int32_t shrink, int64_t *old_rows_out, int64_t *new_size);
/* Drop rows >= new_size: they are cleared as in a never-written store (fp32 rows, norms, both
 * coarse planes, scales, live bits; the scale groups of the 64-row tile that new_size cuts are
 * re-quantised) and size becomes new_size.  new_size > size (or < 0) -> CM_EINVAL.  The last step of
 * cm_dense_compact, and of a sharded compaction on every shard.  No reference counterpart. */
int cm_dense_truncate(cm_dense *h, int64_t new_size);
/* ChromaVectorStore.reset_collection (vector_chroma.py:262-269).  Also clears the int8 plane's centre
 * (cm_dense_set_center): a reset store is a never-written one. */
int cm_dense_reset(cm_dense *h);
/* Centre of the int8 coarse plane (K1q / K1q-s), for anisotropic embeddings (E5-like: every vector
 * near one dominant direction, pairwise cosine 0.7-0.9).  With a centre mu the plane stores
 * q8(xn - mu) and the constant mu.qn is added back exactly per query, so the per-row bound E_r shrinks
 * with ||xn - mu|| while every result stays exact: the f16 plane, the seed and the fp64 re-rank read
 * uncentred data, and results do not depend on mu (only the re-ranked band and the fallbacks do).
 * mu: host array of dim floats, or NULL to clear the centre (the default: the plain plane, bit for
 * bit).  A non-finite entry or ||mu||_2 > 1 -> CM_EINVAL with the handle as it was (a mean of unit
 * vectors never exceeds 1).  Stores mu and re-quantises every written row group on the handle's
 * stream; returns when done; no search or upsert may run concurrently.  On an empty store it only
 * stores mu; later upserts, growth, cm_dense_compact and cm_dense_truncate quantise under it, and
 * cm_dense_compact's shrink keeps it.  Where the automatic kinds are K1c / K1s (other dims,
 * CM_DENSE_Q8=0) the centre is stored and changes no search.  No reference counterpart. */
int cm_dense_set_center(cm_dense *h, const float *mu);
/* The centre: mu_out (nullable, dim floats; zeros when none is set), *is_set (nullable) 1 or 0. */
int cm_dense_get_center(cm_dense *h, float *mu_out, int32_t *is_set);
/* Mean of the normalised live rows of [0, size), the natural centre: column sums of xn = c * invc in
 * fp64 on the device (one pass over the fp32 rows, fixed reduction order: two calls on the same store
 * return the same bits), divided by the live count and rounded to fp32.  mean_out: dim floats;
 * *n_live_out nullable.  No live row -> zeros.  Waits for the device's pending work. */
int cm_dense_mean(cm_dense *h, float *mean_out, int64_t *n_live_out);
/* cm_dense_mean's fp64 column sums (dim doubles) and live count, undivided: what a sharded index adds
 * across its shards before dividing once. */
int cm_dense_column_sums(cm_dense *h, double *sums_out, int64_t *n_live_out);
/* ChromaVectorStore.count (vector_chroma.py:255-260). */
int64_t cm_dense_live_count(cm_dense *h);
int64_t cm_dense_size(cm_dense *h); /* high-water row count */
int32_t cm_dense_dim(cm_dense *h);
/* ChromaVectorStore.query (vector_chroma.py:204-253), batched: for each of
 * nq queries (host, nq x dim) return the k nearest live+allowed rows in
 * ascending (distance, row) order.  out_dist/out_row: nq x k.  out_vec
 * (nullable): nq x k x dim, the stored embeddings (include_embeddings).
 * allow_bits (nullable, host or device memory -- e.g. cm_filter_eval's
 * output, complete before the call): ceil(size/32) words.               */
int cm_dense_search(cm_dense *h, const float *q, int32_t nq, int32_t k, const uint32_t *allow_bits,
                    float *out_dist, int64_t *out_row, float *out_vec);
/* ChromaVectorStore.query (rag/retrieval/vector_chroma.py:204-253) for a batch whose queries carry
 * different where clauses.  allow_bits: n_filters bitmaps of ceil(size/32) words each, one after the
 * other, host or device memory (as cm_dense_search's).  filter_of (host): nq entries in [0, n_filters).
 * Query i gets the k nearest rows that are live and allowed by bitmap filter_of[i], in ascending
 * (distance, row) order.  Distances use cm_dense_search's k > cm_max_topk formula:
 * (float)(1 - c.q / ((|c| + 1e-30)(|q| + 1e-30))) in fp64.  Entries past the allowed live rows are
 * row -1 with the pad distance cm_dense_search writes.  out_vec nullable, as cm_dense_search.
 * Host function: runs on the handle's stream, may synchronise, returns when the outputs are written.
 * No scan: the allowed live rows of every bitmap are compacted into a row list, and only those fp32
 * rows are read, once per tile of 8 queries that share the list.  A null handle or argument, nq < 1,
 * k < 1, n_filters < 1 and a filter_of entry outside [0, n_filters) -> CM_EINVAL, checked on the host
 * before any device call; k > cm_max_topk(), or a batch with 2^31 or more (query, allowed row)
 * pairs -> CM_EUNSUPPORTED; a failed workspace allocation -> CM_ENOMEM. */
int cm_dense_search_lists(cm_dense *h, const float *q, int32_t nq, int32_t k, const uint32_t *allow_bits,
                          int32_t n_filters, const int32_t *filter_of, float *out_dist, int64_t *out_row,
                          float *out_vec);
/* cm_dense_search_lists (ChromaVectorStore.query, rag/retrieval/vector_chroma.py:204-253, per-query
 * where clauses) with the queries and the results on the device: q_dev (nq x dim fp32), dist_dev and
 * row_dev (nq x k) are device memory; allow_bits host or device memory and filter_of host memory, as
 * above.  There is no out_vec: the caller gathers rows itself (cm_dense_gather_dev).  The same body as
 * cm_dense_search_lists and the same bits: the queries are padded and their fp64 norms summed by a
 * device kernel in the host loop's order (one sequential fp64 chain per query, a correctly rounded
 * square root).  Stream contract: the work runs on the handle's own stream behind an event recorded
 * on `stream` (the caller's: a producer of q_dev or allow_bits enqueued on it before the call is
 * waited for on the device); the list lengths are read back as in the host function, so the call
 * synchronises the handle's stream -- never the device -- and the outputs are complete when it
 * returns.  Not graph-capturable.  Argument checks and return codes as cm_dense_search_lists, on the
 * host before any device call. */
int cm_dense_search_lists_dev(cm_dense *h, const float *q_dev, int32_t nq, int32_t k, const uint32_t *allow_bits,
                              int32_t n_filters, const int32_t *filter_of, float *dist_dev, int64_t *row_dev,
                              void *stream);
/* workspace bytes cm_dense_search_dev needs for (nq, k). */
int64_t cm_dense_search_workspace(cm_dense *h, int32_t nq, int32_t k);
/* which scan kernel cm_dense_search[_dev] runs for (nq, k): CM_DENSE_F32
 * (K1, fp32 MFMA, reads 4 B/element: k > 32, other dims, small corpora),
 * CM_DENSE_COARSE (K1c, f16 plane, 2 B/element, 256-query resident passes,
 * certified exact re-rank), CM_DENSE_STREAM (K1s, f16 plane, 2 B/element,
 * nq <= 32, per-wave HBM streams, same re-rank), CM_DENSE_Q8 (K1q, int8 plane
 * with per-row scales, 1 B/element, 256-query resident passes, per-row
 * certified exact re-rank; the automatic choice at dim 768 for nq > 32, unless
 * $CM_DENSE_Q8=0, which keeps K1c / K1s), CM_DENSE_Q8S (below); -1 on error.  Lets callers price the launch against the
 * right roofline.  CM_DENSE_F16X3 (the retired split-plane K1b) is accepted by
 * cm_dense_set_path and means automatic.  */
#define CM_DENSE_F32 1
#define CM_DENSE_F16X3 2
#define CM_DENSE_COARSE 3
#define CM_DENSE_STREAM 4
#define CM_DENSE_Q8 5
/* K1q-s: the int8 plane streamed per wave (register ring, no LDS) for nq <= 32,
 * the same certified re-rank as K1q; the automatic choice at dim 768 for nq <= 32
 * (unless $CM_DENSE_Q8=0, which keeps K1s) */
#define CM_DENSE_Q8S 6
int32_t cm_dense_search_kind(cm_dense *h, int32_t nq, int32_t k);
/* force a scan kernel for this handle (0 = automatic; an ineligible forced
 * kind falls back to the automatic choice).  Results agree within the 1e-4
 * distance tolerance on every path; used for A/B probes and parity tests. */
int cm_dense_set_path(cm_dense *h, int32_t kind);
/* K1c/K1s: number of queries of the search that last used `workspace_dev` whose
 * certificate failed and that were re-run by the exact fp32 pass
 * (synchronous read; 0 for other paths, -1 on error).                    */
int32_t cm_dense_workspace_fallbacks(cm_dense *h, int32_t nq, int32_t k, const void *workspace_dev);
/* same, for the last host-array cm_dense_search on this handle. */
int32_t cm_dense_last_fallbacks(cm_dense *h);
/* K1q/K1q-s: queries of that search whose band overflowed the re-rank's LDS
 * (near-duplicate clusters) and that the wide re-rank finished exactly from
 * the complete candidate buffers instead of the exact scan of every row
 * (ChromaVectorStore.query's result for them is unchanged,
 * rag/retrieval/vector_chroma.py:204-253); 0 for other paths, -1 on error. */
int32_t cm_dense_workspace_wide_reranks(cm_dense *h, int32_t nq, int32_t k, const void *workspace_dev);
int32_t cm_dense_last_wide_reranks(cm_dense *h);
/* K1q/K1q-s: rows whose exact fp64 distance that search's re-rank computed from
 * the fp32 rows, summed over its queries (the certified band, plus the rows of
 * the pilot bound; $CM_K1Q_PILOT=0 forms the band without it, A/B); 0 for
 * other paths, -1 on error.                                              */
int64_t cm_dense_workspace_band_rows(cm_dense *h, int32_t nq, int32_t k, const void *workspace_dev);
int64_t cm_dense_last_band_rows(cm_dense *h);
/* kernel timing (bench roofline): while enabled, every search records HIP
 * events on its launch stream around its scan kernel (K1 / K1c / K1s coarse
 * scan); _drain synchronises on them, writes up to cap elapsed ms values and
 * returns how many were recorded (< 0 on error).                         */
int cm_dense_timing(cm_dense *h, int32_t enable);
/* cm_dense_set_seed_event: a hipEvent_t (NULL clears) recorded on the search stream right after K1q's
 * seed pass of every later batched search -- another stream can start work that should not compete
 * with the seed pass for CUs (bench.py --bm25-gate 2).  The caller keeps the event alive. */
int cm_dense_set_seed_event(cm_dense *h, void *event);
int32_t cm_dense_timing_drain(cm_dense *h, float *ms_out, int32_t cap);
int cm_dense_search_dev(cm_dense *h, const float *q_dev, int32_t nq, int32_t k, const uint32_t *allow_dev,
                        float *dist_dev, int64_t *row_dev, void *workspace_dev, int64_t workspace_bytes,
                        void *stream);
/* cm_dense_search_dev in two parts (same arguments, same stream order): the
 * scan + certified re-rank, then the exact fp32 pass for the queries whose
 * certificate failed (gated on the device: every workgroup leaves at once when
 * none did).  A caller enqueues the second part after its concurrent streams'
 * work has joined (ChromaVectorStore.query, vector_chroma.py:204-253, within
 * HybridRetriever.retrieve, fusion.py:124-125): the exact pass's workgroups ask
 * for ~150 KiB of LDS each and would otherwise wait behind the other stream's
 * kernels.  For CM_DENSE_F32 the first part is the whole search and the second
 * does nothing.  The deferred form also runs K1q with its shared LDS footprint
 * (131 KiB instead of 160: room for one BM25 block beside each scan workgroup);
 * results are identical either way.                                        */
int cm_dense_search_dev_deferred(cm_dense *h, const float *q_dev, int32_t nq, int32_t k, const uint32_t *allow_dev,
                                 float *dist_dev, int64_t *row_dev, void *workspace_dev, int64_t workspace_bytes,
                                 void *stream);
int cm_dense_exact_fallback_dev(cm_dense *h, const float *q_dev, int32_t nq, int32_t k, const uint32_t *allow_dev,
                                float *dist_dev, int64_t *row_dev, void *workspace_dev, int64_t workspace_bytes,
                                void *stream);
/* copy rows [row0, row0+n) to host (n x dim fp32) and/or their live bits
 * (row0 % 32 == 0; ceil(n/32) words).  Persistence and verification. */
int cm_dense_export(cm_dense *h, int64_t row0, int64_t n, float *out, uint32_t *live_out);
/* gather stored rows (row < 0 => zeros): out_dev n x dim. */
int cm_dense_gather_dev(cm_dense *h, const int64_t *rows_dev, int64_t n, float *out_dev, void *stream);
/* device pointer of the live bitmap (ceil(size/32) words) for callers that
 * AND their own filters on device. */
const uint32_t *cm_dense_live_bits_dev(cm_dense *h);

/* BM25 Okapi -------------------------------------------------------------
 * Replaces BM25Store's scoring (rag/retrieval/bm25.py:140-212) and the
 * rank_bm25.BM25Okapi it builds per search (k1=1.5, b=0.75, eps=0.25):
 * CSR postings by term in HBM, term-ordered fp64 accumulation, statistics
 * (N, avgdl, df, idf with the eps floor) over the filtered candidate set.  */
typedef struct cm_bm25 cm_bm25;

int cm_bm25_create(int device, cm_bm25 **out);
void cm_bm25_destroy(cm_bm25 *h);
/* BM25Store._rebuild / BM25Okapi.__init__ (bm25.py:140-145): build from
 * doc-major term ids (host): doc d's tokens are term_ids[doc_off[d] ..
 * doc_off[d+1]) in token order, term ids in [0, vocab).  live (nullable):
 * one byte per doc, 0 = tombstone (deleted, keeps insertion order of the
 * others).  Returns CM_EZERODIV when live docs exist but none has a token
 * (the reference raises ZeroDivisionError there). */
int cm_bm25_build(cm_bm25 *h, const int32_t *term_ids, const int64_t *doc_off, int64_t ndocs, int32_t vocab,
                  const uint8_t *live);
/* same from device arrays (K7: device CSR build by radix sort). */
int cm_bm25_build_dev(cm_bm25 *h, const int32_t *term_ids_dev, const int64_t *doc_off_dev, int64_t ndocs,
                      int64_t ntokens, int32_t vocab, void *stream);
/* BM25Store.upsert_many for ids new to the store (rag/retrieval/bm25.py:147-166): the n_new
 * documents (doc_off[n_new + 1] from 0, term ids in [0, vocab), vocab >= the index's) become
 * rows [ndocs, ndocs + n_new), all live, without a rebuild: their postings are built on the
 * device and merged behind each term's existing ones.  Afterwards the handle equals one that
 * cm_bm25_build made over all documents, old then new, with the old documents' live bytes:
 * exports, statistics and every search, bit for bit.  Local statistics replace any installed
 * with cm_bm25_set_stats; a prepared filter table (cm_bm25_prepare_filtered) grows with the
 * document count.  An index without documents gets the build; n_new == 0 changes nothing.
 * Errors (as cm_bm25_build's; vocab below the index's: CM_EINVAL) leave the handle as it was,
 * except CM_EZERODIV, which cm_bm25_build also reports after the fact.  Peak device memory:
 * old + new postings.  Host semantics as cm_bm25_build (only the new documents are uploaded);
 * _dev as cm_bm25_build_dev: synchronises, not capturable, no search on the handle meanwhile.
 * With cm_bm25_timing on, the merge kernel's time is the next cm_bm25_timing_drain entry.     */
int cm_bm25_append(cm_bm25 *h, const int32_t *term_ids, const int64_t *doc_off, int64_t n_new, int32_t vocab);
int cm_bm25_append_dev(cm_bm25 *h, const int32_t *term_ids_dev, const int64_t *doc_off_dev, int64_t n_new,
                       int64_t ntokens, int32_t vocab, void *stream);
/* BM25Store.delete_many (rag/retrieval/bm25.py:168-172): remove documents and renumber the
 * survivors in order (row r becomes r minus the number of removed rows below it), without a
 * rebuild: a device-side stream compaction of the postings, lengths and live bits.  Afterwards
 * the handle equals cm_bm25_build over the surviving documents with the same vocab (and, for an
 * index built with tombstones, the survivors' live flags): exports, statistics and every search,
 * bit for bit.  rows: n_rows row numbers in [0, ndocs), any order, duplicates allowed (checked on
 * the host: CM_EINVAL).  Local statistics replace any installed with cm_bm25_set_stats; a
 * prepared filter table is kept.  n_rows == 0 changes nothing; removing every document leaves
 * the build of none.  CM_EINVAL and CM_ENOMEM leave the handle as it was; CM_EZERODIV (live
 * documents remain but no token) is reported with the new state installed, as a build of those
 * documents reports it.  Peak device memory: old + new postings plus 16 B per 64 postings.
 * Synchronises, not capturable, no search on the handle meanwhile.  With cm_bm25_timing on, the
 * two compaction passes' times are the next two cm_bm25_timing_drain entries.                  */
int cm_bm25_remove(cm_bm25 *h, const int64_t *rows, int64_t n_rows);
/* The same from a device bitmap: bit r of remove_bits_dev set = remove row r
 * (ceil(ndocs / 32) words; bits at or above ndocs are ignored; no bit set changes nothing). */
int cm_bm25_remove_dev(cm_bm25 *h, const uint32_t *remove_bits_dev, void *stream);
/* BM25Store.upsert_many for ids the store already holds (rag/retrieval/bm25.py:147-166: the dict
 * assignment keeps the document's row): document i, the tokens term_ids[doc_off[i] .. doc_off[i+1])
 * (doc_off[0] == 0, term ids in [0, vocab), vocab >= the index's: new terms may arrive with the
 * replacement), takes the place of row rows[i], without a rebuild: the replaced rows' postings are
 * dropped and the new texts' postings, built on the device, are scattered between each term's
 * surviving ones.  Afterwards the handle equals cm_bm25_build over the same documents with those
 * rows substituted and the same vocab; the replaced rows are live, every other row keeps its live
 * flag (tombstones of a build with `live` included): exports, cm_bm25_stats, cm_bm25_term_stats,
 * the head-term count and every search, bit for bit.  rows: n_rows distinct row numbers in
 * [0, ndocs), any order (a duplicate or out-of-range row: CM_EINVAL, checked on the host; the host
 * sorts the documents by row before upload).  Local statistics replace any installed with
 * cm_bm25_set_stats; a prepared filter table is kept; ndocs does not change.  n_rows == 0 changes
 * nothing.  CM_EINVAL, CM_ENOMEM and CM_EUNSUPPORTED (a tf above 65535) leave the handle as it
 * was; CM_EZERODIV (live documents but no token) is reported with the new state installed, as
 * cm_bm25_remove does.  Peak device memory: old + new postings, 16 B per 64 postings, the delta
 * and its sort scratch.  Synchronises, not capturable, no search on the handle meanwhile.  With
 * cm_bm25_timing on, the flag pass with its scan and the scatter passes are the next two
 * cm_bm25_timing_drain entries.                                                               */
int cm_bm25_replace(cm_bm25 *h, const int64_t *rows, int64_t n_rows, const int32_t *term_ids, const int64_t *doc_off,
                    int32_t vocab);
/* The same from device arrays (ntokens = doc_off_dev[n_rows]).  rows_dev must be strictly
 * ascending and within [0, ndocs): checked on the device, with a flag read back before anything
 * is modified (CM_EINVAL). */
int cm_bm25_replace_dev(cm_bm25 *h, const int64_t *rows_dev, int64_t n_rows, const int32_t *term_ids_dev,
                        const int64_t *doc_off_dev, int64_t ntokens, int32_t vocab, void *stream);
int64_t cm_bm25_num_docs(cm_bm25 *h);
int64_t cm_bm25_num_postings(cm_bm25 *h);
/* unfiltered corpus statistics: live docs, total length, avgdl, eps. */
int cm_bm25_stats(cm_bm25 *h, int64_t *n_live, int64_t *sum_len, double *avgdl, double *eps);
/* Dense head-term tiles (K2 fast path): terms with df > ndocs * min_df_frac
 * (highest df first, at most max_bytes of uint8 tf tiles) are scored from a
 * [term][doc] tf tile instead of their postings.  Default 1/64 and 8 GiB;
 * max_bytes = 0 disables.  Results are identical either way. */
int cm_bm25_set_head_policy(cm_bm25 *h, double min_df_frac, int64_t max_bytes);
int32_t cm_bm25_num_head_terms(cm_bm25 *h);
/* Search strategy (results are identical on both):
 *   CM_BM25_FULL   K2 scores every (query, 1024-doc range) pair;
 *   CM_BM25_PRUNED K2a scores the documents holding a tail (non-head) query
 *                  term, then K2 re-scores only the (query, range) pairs whose
 *                  head-only score bound reaches the query's k-th best tail
 *                  score.  0 = automatic (pruned).          */
#define CM_BM25_FULL 1
#define CM_BM25_PRUNED 2
int cm_bm25_set_path(cm_bm25 *h, int32_t kind);
/* (query, range) pairs K2 re-scored by the pruned search that last used
 * `workspace_dev` (synchronous read; -1 on the full path or error), and the
 * same for the last host-array cm_bm25_search on this handle.            */
int32_t cm_bm25_workspace_rescored(cm_bm25 *h, int32_t nq, int32_t total_terms, int32_t k, const void *workspace_dev);
int32_t cm_bm25_last_rescored(cm_bm25 *h);
/* K2b's planned items of the pruned search that last used `workspace_dev` (synchronous read):
 * returns their count (-1 on the full path or error) and copies up to cap items (q << 40 |
 * 1024-doc range << 16 | 64-doc block mask) -- bench.py prices K2b's algorithmic bytes with them. */
int64_t cm_bm25_workspace_items(cm_bm25 *h, int32_t nq, int32_t total_terms, int32_t k, const void *workspace_dev,
                                uint64_t *items_out, int64_t cap);
/* the same items' planned 16-doc sub-blocks (bit 4 b + x = sub-block x of 64-doc block b of the
 * item's range; round 6: K2b scores only these) -- item i's mask is masks_out[i].  New: the planner
 * refines the reference-free block plan above, so no reference interface corresponds to it. */
int64_t cm_bm25_workspace_subblocks(cm_bm25 *h, int32_t nq, int32_t total_terms, int32_t k, const void *workspace_dev,
                                    uint64_t *masks_out, int64_t cap);
/* kernel timing (bench roofline): events around every search's K2 launch;
 * same contract as cm_dense_timing / cm_dense_timing_drain.              */
int cm_bm25_timing(cm_bm25 *h, int32_t enable);
int32_t cm_bm25_timing_drain(cm_bm25 *h, float *ms_out, int32_t cap);
/* the same for K2b (bm25_block_kernel) launches of the pruned search. */
int32_t cm_bm25_timing_drain_block(cm_bm25 *h, float *ms_out, int32_t cap);
/* Sharding support: local df per term and the first posting's
 * (row << 32 | first position) key (0xff..ff when absent), so ranks can
 * all-reduce df (sum) and first keys (min, after offsetting rows) and agree
 * on the reference's dict order; then install the global statistics. */
/* copy the device index to host (any pointer may be NULL): term_off[V+1],
 * post_doc/post_tf/post_pos[P], dl[N]. */
int cm_bm25_export(cm_bm25 *h, int64_t *term_off, int32_t *post_doc, uint16_t *post_tf, uint32_t *post_pos,
                   int32_t *dl);
int cm_bm25_term_stats(cm_bm25 *h, int32_t *df_out, uint64_t *first_out);
int cm_bm25_set_stats(cm_bm25 *h, const double *idf, int32_t vocab, int64_t n_live, int64_t sum_len, double eps);
/* BM25Store.search (bm25.py:175-212) batched: nq queries whose term ids
 * (host, -1 = unknown term) are q_terms[q_off[i] .. q_off[i+1]) in query
 * token order (duplicates count twice).  Candidates = live docs with the
 * allow bit set; statistics are recomputed over them when allow_bits is
 * given (quirk Q2).  Output per query: k (score, row) in descending score,
 * ties -> lower row, zero-score docs padding in row order (quirk Q1);
 * out_n[i] = number of valid entries (min(k, #candidates)).               */
int cm_bm25_search(cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off, int32_t nq, int32_t k,
                   const uint32_t *allow_bits, double *out_score, int64_t *out_row, int32_t *out_n);
/* BM25Store.search for a batch whose queries carry different where clauses.  q_terms, q_off and
 * the outputs as cm_bm25_search; allow_bits: n_filters bitmaps of ceil(ndocs/32) words each, one after
 * the other, host or device memory; filter_of (host): nq entries in [0, n_filters).  Query i's
 * result is bit for bit cm_bm25_search's for that query alone under bitmap filter_of[i]: scores,
 * rows, out_n[i] = min(k, Nc) and the (0.0, -1) pads; descending score, ties -> lower row,
 * zero-score candidates padding in row order (quirk Q1); statistics (Nc, avgdl, df, the epsilon
 * floor) of each bitmap's own candidate set (quirk Q2).  Any k >= 1: the result is a full order.
 * Host function: runs on the handle's stream, synchronises, returns when the outputs are written.
 * No scan and no posting walk: the allowed live rows of every bitmap are compacted into a row list,
 * and each (query, row) pair is scored outright, its tf looked up in the term's head tile or by a
 * binary search of its postings; one segmented sort orders every query's candidates (DESIGN §3
 * "BM25 row-list search").  Only the bitmaps with a negative idf need their epsilon, and up to 32 of
 * them share one pass over all postings (cm_bm25_filter_eps_multi's);
 * cm_bm25_last_eps_filters = how many of the last call's did (-1: null handle).
 * A null handle or argument, nq < 1, k < 1, n_filters < 1, a filter_of entry outside [0, n_filters)
 * and a decreasing q_off -> CM_EINVAL, checked on the host before any device call; 2^31 or more
 * (query, allowed row) pairs, or n_filters x ceil(ndocs/32) words -> CM_EUNSUPPORTED; a bitmap some
 * query uses whose candidates hold no tokens -> CM_EZERODIV (cm_bm25_search's message); a failed
 * workspace allocation -> CM_ENOMEM.  The handle stays usable after every error. */
int cm_bm25_search_lists(cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off, int32_t nq, int32_t k,
                         const uint32_t *allow_bits, int32_t n_filters, const int32_t *filter_of,
                         double *out_score, int64_t *out_row, int32_t *out_n);
/* cm_bm25_search_lists (BM25Store.search, rag/retrieval/bm25.py:175-212, per-query where clauses)
 * with the results on the device: score_dev and row_dev (nq x k) are device memory; q_terms, q_off,
 * filter_of and out_n stay on the host (tokenising is host work; out_n is known after the first
 * read-back), allow_bits host or device memory.  The same body and the same bits.
 * eps_io (nullable, host, n_filters doubles): the epsilon floors the caller already knows.  NaN on
 * entry = not known (0.0 is a legitimate floor).  A bitmap that turns out to have a negative idf uses
 * its eps_io value when it has one and joins no postings pass; with NaN its floor is computed as in
 * the host function and written back.  A bitmap without a negative idf in this call is left
 * untouched.  cm_bm25_last_eps_filters / cm_bm25_last_eps_passes count only what was computed.
 * Stream contract: the work runs on the handle's own stream behind an event recorded on `stream`
 * (the caller's: a producer of allow_bits enqueued on it before the call is waited for on the
 * device); the call keeps the host function's read-backs, so it synchronises the handle's stream --
 * never the device -- and the outputs are complete when it returns.  Not graph-capturable.
 * Argument checks and return codes as cm_bm25_search_lists, on the host before any device call. */
int cm_bm25_search_lists_dev(cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off, int32_t nq, int32_t k,
                             const uint32_t *allow_bits, int32_t n_filters, const int32_t *filter_of, double *eps_io,
                             double *score_dev, int64_t *row_dev, int32_t *out_n, void *stream);
int32_t cm_bm25_last_eps_filters(cm_bm25 *h);
/* cm_bm25_search with the caller's statistics instead of this index's: q_idf[total] = every
 * query term's idf (0 for terms outside the candidate vocabulary; ignored for ids outside
 * [0, vocab)), avgdl and n_cand of the candidate set; allow_bits (host or device words,
 * nullable) restricts the scored documents.  A corpus sharded over several devices in one process
 * (classmate_hip/multidev.py, SURVEY §8(b) Threading / §8(e)) scores every shard with the GLOBAL
 * statistics -- for a where-filter the statistics of the filtered candidates of all shards (quirk
 * Q2, rag/retrieval/bm25.py:184-191) -- and merges the shards' lists by (score desc, row asc).
 * n_cand may therefore exceed this index's own candidates (its live docs with the allow bit set):
 * the output then holds only those, every further entry is (score 0.0, row -1), and out_n[i]
 * counts the entries of query i with row >= 0 (local valid entries, not min(k, n_cand)). */
int cm_bm25_search_idf(cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off, int32_t nq, int32_t k,
                       const uint32_t *allow_bits, const double *q_idf, double avgdl, int64_t n_cand,
                       double *out_score, int64_t *out_row, int32_t *out_n);
/* unfiltered device variant (inputs and outputs device, graph-capturable). */
int64_t cm_bm25_search_workspace(cm_bm25 *h, int32_t nq, int32_t total_terms, int32_t k);
int cm_bm25_search_dev(cm_bm25 *h, const int32_t *q_terms_dev, const int32_t *q_off_dev, int32_t nq,
                       int32_t total_terms, int32_t k, double *score_dev, int64_t *row_dev,
                       void *workspace_dev, int64_t workspace_bytes, void *stream);
/* the same search with its scoring kernels behind gate_event (a hipEvent_t, NULL = none): the
 * query preparation (term descriptors, postings bounds, the seeded threshold) runs at once, beside
 * the caller's producer work (HybridRetriever.retrieve encodes the query first,
 * rag/retrieval/fusion.py:124-125), the tail pass and everything after it wait for the event.
 * Results are identical. */
int cm_bm25_search_dev_gated(cm_bm25 *h, const int32_t *q_terms_dev, const int32_t *q_off_dev, int32_t nq,
                             int32_t total_terms, int32_t k, double *score_dev, int64_t *row_dev,
                             void *workspace_dev, int64_t workspace_bytes, void *stream, void *gate_event);

/* Filtered search on the device (quirk Q2: rank_bm25 statistics over the
 * candidate set, rag/retrieval/bm25.py:184-191), graph-capturable.
 *   cm_bm25_prepare_filtered: host call, once per index (before capture):
 *     uploads L[x] = log(x + 0.5) for x <= max(max_docs, num_docs) (glibc,
 *     CPython's math.log), so the device forms idf = L[Nc - df] - L[df] with
 *     rank_bm25's exact bits.  max_docs = the global corpus size on a shard.
 *   cm_bm25_filter_stats_dev: stats_dev = {Nc, sum of candidate lengths}
 *     (int64[2]), df_dev[i] = candidate df of q_terms_dev[i] (int64).  A
 *     sharded index all-reduces (sums) both before searching.
 *   cm_bm25_filter_term_stats_dev: the same for every term (df int64[V]) plus
 *     each term's first candidate (row << 32 | position) key (uint64[V],
 *     ~0 = none): a shard's share of the epsilon floor's statistics.
 *   cm_bm25_filter_eps: host call; rank_bm25's epsilon (0.25 x the mean idf
 *     of the candidate vocabulary in first-occurrence order) for one filter;
 *     allow_bits host or device words.
 *   cm_bm25_search_stats_dev: cm_bm25_search_dev over the allowed documents
 *     with the given candidate statistics; eps_dev (nullable) is the epsilon
 *     used when an idf is negative.  status_dev (int32, written on stream):
 *     bit 0 an idf was negative and eps_dev was NULL/NaN (compute eps with
 *     cm_bm25_filter_eps and search again), bit 1 candidates without tokens
 *     (the reference's ZeroDivisionError), bit 2 Nc beyond the prepared table.
 *   cm_bm25_search_filtered_dev: filter_stats_dev + search_stats_dev on one
 *     index (workspace: cm_bm25_search_workspace).                          */
int cm_bm25_prepare_filtered(cm_bm25 *h, int64_t max_docs);
int cm_bm25_filter_stats_dev(cm_bm25 *h, const uint32_t *allow_dev, const int32_t *q_terms_dev, int32_t n_terms,
                             int64_t *stats_dev, int64_t *df_dev, void *stream);
int cm_bm25_filter_term_stats_dev(cm_bm25 *h, const uint32_t *allow_dev, int64_t *df_dev, uint64_t *first_dev,
                                  void *stream);
int cm_bm25_filter_eps(cm_bm25 *h, const uint32_t *allow_bits, double *eps_out);
/* cm_bm25_filter_eps for n_filters bitmaps at once: eps_out[f] (host, n_filters doubles) is bit for
 * bit what cm_bm25_filter_eps returns for bitmap f (0.0 for a bitmap without candidates).
 * allow_bits: n_filters bitmaps of ceil(ndocs/32) words each, one after the other, host or device
 * memory.  Up to 32 bitmaps share one pass over the postings (a 32-bit membership word per
 * document); the candidate vocabulary, its first-occurrence order, the idfs and the sequential
 * fp64 sum stay on the device, and one (sum, count) pair per bitmap is read back (DESIGN §3 "BM25
 * epsilon floors, 32 clauses a pass").  Host function: runs on the handle's stream, synchronises.
 * A null argument or n_filters < 0 -> CM_EINVAL; n_filters == 0 -> CM_OK, nothing done; n_filters x
 * ceil(ndocs/32) >= 2^31 - 1 words -> CM_EUNSUPPORTED (all checked before any device call); a bitmap
 * whose candidates hold no tokens -> CM_EZERODIV (cm_bm25_filter_eps' message); a failed workspace
 * allocation -> CM_ENOMEM.  The handle stays usable after every error. */
int cm_bm25_filter_eps_multi(cm_bm25 *h, const uint32_t *allow_bits, int32_t n_filters, double *eps_out);
/* Postings passes (rounds of up to 32 bitmaps) taken by the last cm_bm25_filter_eps_multi or
 * cm_bm25_search_lists call on the handle; -1 for a null handle. */
int32_t cm_bm25_last_eps_passes(cm_bm25 *h);
int cm_bm25_search_stats_dev(cm_bm25 *h, const int32_t *q_terms_dev, const int32_t *q_off_dev, int32_t nq,
                             int32_t total_terms, int32_t k, const uint32_t *allow_dev, const int64_t *stats_dev,
                             const int64_t *df_dev, const double *eps_dev, double *score_dev, int64_t *row_dev,
                             int32_t *status_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int cm_bm25_search_filtered_dev(cm_bm25 *h, const int32_t *q_terms_dev, const int32_t *q_off_dev, int32_t nq,
                                int32_t total_terms, int32_t k, const uint32_t *allow_dev, const double *eps_dev,
                                double *score_dev, int64_t *row_dev, int32_t *status_dev, void *workspace_dev,
                                int64_t workspace_bytes, void *stream);

/* Where-filters on the device ---------------------------
 * A where clause compiled on the host (classmate_hip/retrieval/filters.py,
 * replacing the per-row _matches_filter of rag/retrieval/bm25.py:79-107
 * and Chroma's where evaluation behind vector_chroma.py:45-78,204-253)
 * into a postfix program: n_ops triples (opcode, a, b) in prog (host).
 *   CM_FOP_EQ / CM_FOP_NE  push cols_dev[a][row] == b  /  != b
 *   CM_FOP_BITS            push bit row of bitmap bits_dev[a]
 *   CM_FOP_TRUE / FALSE    push a constant
 *   CM_FOP_AND / OR        pop two, push the result;  CM_FOP_NOT  negate top
 * cols_dev / bits_dev: host arrays of device pointers (int32 value codes,
 * n_rows each; uint32 bitmaps, ceil(n_rows/32) words).  out_dev receives
 * ceil(n_rows/32) words (bit r & 31 of word r >> 5); count_dev (nullable,
 * device) the number of set bits.  Stack depth <= 32; <= CM_FILTER_MAX_OPS
 * ops and <= CM_FILTER_MAX_SOURCES columns and bitmaps.  Async on stream. */
#define CM_FILTER_MAX_OPS 64
#define CM_FILTER_MAX_SOURCES 16
#define CM_FOP_EQ 1
#define CM_FOP_NE 2
#define CM_FOP_BITS 3
#define CM_FOP_TRUE 4
#define CM_FOP_FALSE 5
#define CM_FOP_AND 6
#define CM_FOP_OR 7
#define CM_FOP_NOT 8
int cm_filter_eval(const int32_t *prog, int32_t n_ops, const int32_t *const *cols_dev, int32_t n_cols,
                   const uint32_t *const *bits_dev, int32_t n_bits, int64_t n_rows, uint32_t *out_dev,
                   unsigned long long *count_dev, void *stream);

/* Fusion -------------------------------------------------------------- */
/* _mmr_order (rag/retrieval/fusion.py:39-61) for nq queries at once:
 * q: nq x dim, cands: nq x pool x dim (fp32), n_valid[i] <= pool rows valid
 * for query i.  out_order: nq x k indices into the pool (-1 pad).         */
int cm_mmr(const float *q, const float *cands, const int32_t *n_valid, int32_t nq, int32_t pool, int32_t dim,
           int32_t k, double lambd, int32_t *out_order);
int cm_mmr_dev(const float *q_dev, const float *cands_dev, const int32_t *n_valid_dev, int32_t nq, int32_t pool,
               int32_t dim, int32_t k, double lambd, int32_t *order_dev, void *stream);
/* rrf_fuse (rag/retrieval/fusion.py:17-36): nl rank lists of int64 keys
 * (host; list i = keys[off[i] .. off[i+1])).  out_keys/out_score receive
 * the distinct keys in first-appearance order (Python dict order) and
 * their fused scores; *out_n = count.  weights nullable (all 1.0).      */
int cm_rrf_fuse(const int64_t *keys, const int32_t *off, int32_t nl, const double *weights, int32_t rrf_k,
                int64_t *out_keys, double *out_score, int32_t *out_n);
/* HybridRetriever.retrieve merge (fusion.py:132-167), batched on device:
 * per query a vector list (<= kv keys with fp32 distance, MMR order) and a
 * BM25 list (<= kb keys with fp64 score); outputs the top_k items sorted by
 * (fused, -distance or -0.0) descending, stable (vector items first).
 * out_flags bit0 = has vector distance, bit1 = has BM25 score.           */
/* Inputs of cm_rrf_merge_dev from the device search outputs (fusion.py:132-153's vec_ids /
 * bm_ids lists): vkeys/vdist[q][i] = pool_keys/pool_dist[q][order[q][i]] for the MMR order
 * (-1 / 0 past the selected count), vn[q] = selected count, bn[q] = valid BM25 rows (>= 0).  */
int cm_rrf_pool_prep_dev(const int64_t *pool_keys, const float *pool_dist, int32_t pool, const int32_t *order,
                         int32_t kv, const int64_t *bkeys, int32_t kb, int32_t nq, int64_t *vkeys, float *vdist,
                         int32_t *vn, int32_t *bn, void *stream);
int cm_rrf_merge_dev(const int64_t *vkeys, const float *vdist, const int32_t *vn, int32_t kv,
                     const int64_t *bkeys, const double *bscore, const int32_t *bn, int32_t kb, int32_t nq,
                     double w_vec, double w_bm25, int32_t rrf_k, int32_t top_k, int64_t *out_keys,
                     double *out_fused, float *out_vdist, double *out_bscore, int32_t *out_flags,
                     int32_t *out_n, void *stream);
int cm_rrf_merge(const int64_t *vkeys, const float *vdist, const int32_t *vn, int32_t kv, const int64_t *bkeys,
                 const double *bscore, const int32_t *bn, int32_t kb, int32_t nq, double w_vec, double w_bm25,
                 int32_t rrf_k, int32_t top_k, int64_t *out_keys, double *out_fused, float *out_vdist,
                 double *out_bscore, int32_t *out_flags, int32_t *out_n);

/* E5 pooling ------------------------------------------------------------
 * sentence-transformers Pooling(mean) + Normalize as used by
 * E5MultilingualEmbedder.encode_* (rag/embeddings/__init__.py:85-105):
 * out[b] = sum_s h[b,s]*m[b,s] / max(sum_s m[b,s], 1e-9), then (if
 * normalize) out[b] /= max(||out[b]||_2, 1e-12).  hidden: B x S x D of
 * hidden_dtype (F32/BF16/F16), mask: B x S of mask_dtype (I32/I64),
 * out: B x D fp32.  All device pointers, torch's stream.                 */
int cm_meanpool_l2norm(const void *hidden_dev, int32_t hidden_dtype, const void *mask_dev, int32_t mask_dtype,
                       int32_t B, int32_t S, int32_t D, int32_t normalize, float *out_dev, void *stream);

/* E5 encoder block epilogue ----------------------------------------------
 * XLM-R "residual add + LayerNorm" (HF XLMRobertaSelfOutput / XLMRobertaOutput /
 * XLMRobertaEmbeddings, run by E5MultilingualEmbedder.encode_*,
 * rag/embeddings/__init__.py:85-105) fused into one pass:
 * out[i] = LN(round(x[i] + r[i % r_rows])) * gamma + beta over D features,
 * fp32 statistics.  r may be NULL (plain LayerNorm); out may alias x.
 * dtype F32 or BF16 for x, r, gamma, beta and out; rows x D row-major.  */
int cm_add_layernorm(const void *x_dev, const void *r_dev, int64_t r_rows, const void *gamma_dev,
                     const void *beta_dev, int64_t rows, int32_t D, float eps, int32_t dtype, void *out_dev,
                     void *stream);

/* Self-attention of an unpadded short batch (HF XLMRobertaSelfAttention with an all-ones
 * mask, as run by E5MultilingualEmbedder.encode_queries): qkv_dev is the fused Q/K/V
 * projection output B x S x 3 x H x head_dim, out_dev receives softmax(q k^T * scale) v as
 * B x S x (H * head_dim).  head_dim must be 64, 0 < S <= 64; dtype F32 or BF16.   */
int cm_short_attention(const void *qkv_dev, int32_t B, int32_t S, int32_t H, int32_t head_dim, float scale,
                       int32_t dtype, void *out_dev, void *stream);

/* fp32-accurate E5 projections on the f16 matrix cores (K10) ------------
 * The XLM-R linear layers y = x W^T + b that E5MultilingualEmbedder.encode_*
 * runs in fp32 (rag/embeddings/__init__.py:85-105, sentence-transformers on
 * torch fp32: nn.Linear in XLMRobertaSelfAttention / SelfOutput /
 * Intermediate / Output), computed as split-precision f16 products: every
 * fp32 operand v = hi + lo (two f16 halves, 22 significant bits), product =
 * lo.hi + hi.lo + hi.hi accumulated in fp32 by v_mfma_f32_16x16x32_f16.
 *
 * "Planes": an M x K fp32 matrix as ONE buffer of 2 KiB split blocks, block
 * (row / 16, k / 32) = [hi halves 1 KiB][lo halves 1 KiB], each in fragment-
 * major order (lane slot c + 16 g = row 16 b + c, k = 32 kb + 8 g .. + 7).
 * A buffer holds cm_f16x3_plane_rows(M) rows (M rounded up to 384, so the
 * GEMM's last tile reads in bounds) x K x 2 halves.  Values are stored times a
 * power-of-two scale with |v * scale| <= 2^15.
 *
 * cm_f16x3_split_rows: fp32 rows (device, M x K row-major) * scale -> planes.
 * cm_f16x3_split_weights: the same for an nn.Linear weight (N x K), once per
 *   model; scale puts max|W| at 2^14..2^15.  N % 16 == 0, K % 32 == 0.
 * cm_linear_f16x3: C = (A planes)(W planes)^T * out_scale + bias, where
 *   out_scale = 1 / (A scale * W scale), bias may be NULL (N <= 4096);
 *   epilogue CM_EPI_BIAS / CM_EPI_BIAS_GELU (exact erf, torch's F.gelu
 *   default) write c_dev (M x N fp32 row-major); CM_EPI_PLANES_GELU writes
 *   GELU(C) * next_scale as planes (c_planes, cm_f16x3_plane_rows(M) x N) for
 *   the next projection (FFN-up -> FFN-down).  K % 64 == 0, N % 64 == 0, any M.
 * cm_add_layernorm_split: cm_add_layernorm (fp32) that also writes its output
 *   rows * a_scale as planes.  D % 32 == 0.
 * cm_short_attention_split: cm_short_attention (fp32) writing the context
 *   * a_scale as planes (B*S x H*64) instead of fp32 rows.
 * cm_short_attention_split_masked: the same for padded batches (S <= 32):
 *   key_mask_dev (B x S int32, nonzero = attend) removes padded keys from
 *   the softmax, as XLM-R's extended attention mask (the reference's HF
 *   forward for a padded query batch, rag/embeddings/__init__.py:85-105).  */
#define CM_EPI_BIAS 0
#define CM_EPI_BIAS_GELU 1
#define CM_EPI_PLANES_GELU 2
/* CM_EPI_PLANES_QKV: the fused QKV projection (N = 3 x H x 64, N % 96 == 0, M > 32) written as planes
 * of C * next_scale for cm_planes_attention: the Q and K thirds in the standard layout, the V third
 * transposed per 32-row unit (the attention's P V operand; see cm_gemm.hip k10_epilogue). */
#define CM_EPI_PLANES_QKV 3
int64_t cm_f16x3_plane_rows(int64_t M);
int cm_f16x3_split_rows(const float *x_dev, int64_t M, int32_t K, float scale, void *planes_dev, void *stream);
int cm_f16x3_split_weights(const float *w_dev, int32_t N, int32_t K, float scale, void *planes_dev, void *stream);
int cm_linear_f16x3(const void *a_planes, int64_t M, int32_t K, const void *w_planes, const float *bias_dev,
                    float out_scale, int32_t N, int32_t epilogue, float *c_dev, float next_scale, void *c_planes,
                    void *stream);
int cm_add_layernorm_split(const float *x_dev, const float *r_dev, int64_t r_rows, const float *gamma_dev,
                           const float *beta_dev, int64_t rows, int32_t D, float eps, float *out_dev, float a_scale,
                           void *planes_dev, void *stream);
int cm_short_attention_split(const float *qkv_dev, int32_t B, int32_t S, int32_t H, int32_t head_dim, float scale,
                             float a_scale, void *planes_dev, void *stream);
int cm_short_attention_split_masked(const float *qkv_dev, int32_t B, int32_t S, int32_t H, int32_t head_dim,
                                    float scale, float a_scale, const int32_t *key_mask_dev, void *planes_dev,
                                    void *stream);
/* cm_long_attention_split: the same context planes for any 0 < S <= 4096 (passages; K9L, a
 * flash-style split-precision MFMA kernel: 64-key chunks through LDS, online softmax in fp32);
 * key_mask_dev (B x S int32, nonzero = attend) may be NULL (every key attends).  Replaces torch
 * SDPA + cm_f16x3_split_rows for the reference's passage encode (rag/embeddings/__init__.py:96-105,
 * truncation at 512 tokens). */
int cm_long_attention_split(const float *qkv_dev, int32_t B, int32_t S, int32_t H, int32_t head_dim, float scale,
                            float a_scale, const int32_t *key_mask_dev, void *planes_dev, void *stream);
/* cm_planes_attention: the same context planes from the CM_EPI_PLANES_QKV output of the QKV
 * projection (qkv_planes = planes of (B*S) x 3*H*64 values times s_qkv, a power of two): K9P, every
 * operand streamed as split blocks by LDS-DMA (the passage encode, S % 64 == 0, S <= 512; the
 * caller pads other lengths with masked keys). */
int cm_planes_attention(const void *qkv_planes, int32_t B, int32_t S, int32_t H, int32_t head_dim, float scale,
                        float s_qkv, float a_scale, const int32_t *key_mask_dev, void *planes_dev, void *stream);

/* The N > 1 step's exchange merge (no reference interface: the reference is single
 * process -- this is the sharded form of ChromaVectorStore.query, vector_chroma.py:204-253, and
 * BM25Store.search's sorted(...)[:top_k], bm25.py:199).  allp_dev: the all-gathered packed shard
 * lists, ws x B x (2P + 2K) int64 (P f32 distance words, P global rows, K f64 score words, K global
 * rows; -1 rows pad).  Writes the global dense top-P (distance asc, row asc) and BM25 top-K
 * (score desc, row asc, -0.0 == 0.0), pads last; device pointers, stream-ordered, no sync.
 * ws x P and ws x K <= 4096. */
int cm_shard_merge_topk_dev(const int64_t *allp_dev, int32_t ws, int32_t B, int32_t P, int32_t K, float *d_out,
                            int64_t *r_out, double *s_out, int64_t *br_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CLASSMATE_HIP_H */
