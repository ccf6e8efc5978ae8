// What cm_bm25_append, cm_bm25_remove and cm_bm25_replace share (included by cm_bm25.hip before
// the three).  Each of them changes the device index without a rebuild, by the same plan:
//   1. a delta CSR of the new documents (bm25_csr_from_tokens) and/or the survivors of the old
//      postings (bm25_survivor_pass);
//   2. the new term offsets, term_off'[t] = surv(term_off[min(t, V_old)]) + d_off[t]
//      (bm25_mut_offsets_kernel; surv is the identity without a removal, d_off 0 without a delta);
//   3. six fresh arrays (FreshArrays), filled by the mutation's own kernels;
//   4. the swap into the handle, once nothing can fail any more, the counts, and K7's second half
//      (bm25_install), which makes the handle bit-equal to one built over the final documents.
// The host forms check their arguments here too (bm25_checked_ntok, bm25_rows_to_bits).

namespace cm {

constexpr int kRmThreads = 256;
constexpr int kRmGroups = 8;  // 64-posting groups per wave
constexpr int64_t kRmChunk = (int64_t)(kRmThreads / 64) * kRmGroups * 64;  // postings per workgroup

// largest t in [a, b] with off[t] <= p; the caller guarantees off[a] <= p < off[b + 1]
__device__ inline int32_t bm25_term_at(const int64_t *__restrict__ off, int32_t a, int32_t b, int64_t p) {
  while (a < b) {
    const int32_t m = a + (b - a + 1) / 2;
    if (off[m] <= p)
      a = m;
    else
      b = m - 1;
  }
  return a;
}

// Pass A: smask[g] = survivors among postings [64 g, 64 g + 64), cnt[g] = their number.
__global__ void __launch_bounds__(kRmThreads) bm25_rm_flag_kernel(const int32_t *__restrict__ post_doc, int64_t npost,
                                                                  const uint32_t *__restrict__ keep,
                                                                  unsigned long long *__restrict__ smask,
                                                                  int64_t *__restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t g0 = ((int64_t)blockIdx.x * (kRmThreads / 64) + (threadIdx.x >> 6)) * kRmGroups;
#pragma unroll
  for (int u = 0; u < kRmGroups; ++u) {
    const int64_t g = g0 + u, p = g * 64 + lane;  // (g is wave-uniform)
    if (g * 64 >= npost) break;
    bool s = false;
    if (p < npost) {
      const int32_t d = post_doc[p];
      s = (keep[d >> 5] >> (d & 31)) & 1u;
    }
    const unsigned long long m = __ballot(s);
    if (lane == 0) {
      smask[g] = m;
      cnt[g] = (int64_t)__popcll(m);
    }
  }
}

// the number of old postings that survive before old posting p (p <= npost): O(1), whatever the term
__device__ inline int64_t bm25_surv(int64_t p, int64_t npost, int64_t p_surv,
                                    const unsigned long long *__restrict__ smask,
                                    const int64_t *__restrict__ sbase) {
  return p >= npost ? p_surv : sbase[p >> 6] + (int64_t)__popcll(smask[p >> 6] & ((1ull << (p & 63)) - 1ull));
}

// term_off'[t] for t in [0, v_new].  smask == NULL: every old posting survives (the append; an index
// without postings); d_off == NULL: no delta (the removal).
__global__ void bm25_mut_offsets_kernel(const int64_t *__restrict__ old_off, int32_t v_old, int32_t v_new,
                                        int64_t npost, int64_t p_surv, const unsigned long long *__restrict__ smask,
                                        const int64_t *__restrict__ sbase, const int64_t *__restrict__ d_off,
                                        int64_t *__restrict__ new_off) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > v_new) return;
  const int64_t p = old_off[t < v_old ? t : v_old];
  new_off[t] = (smask ? bm25_surv(p, npost, p_surv, smask, sbase) : p) + (d_off ? d_off[t] : 0);
}

}  // namespace cm

namespace {

// The survivors of the old postings under the keep words: bit p & 63 of smask[p >> 6] is posting
// p's, sbase[g] the survivors before group g, n their total.  Both arrays stay empty when the index
// has no postings.
struct Survivors {
  TmpBuf smask, sbase;
  int64_t n = 0;
  const unsigned long long *mask() const { return smask.as<unsigned long long>(); }
  const int64_t *base() const { return sbase.as<int64_t>(); }
};

// Pass A and its scan (in place, over the group counts and one zero behind them), one
// cm_bm25_timing pair; the total is read back (a synchronise of `st`).
int bm25_survivor_pass(cm_bm25 *h, const uint32_t *keep, TmpBuf &cub_tmp, Survivors &s, hipStream_t st) {
  const int64_t p0 = h->npost, ng = ceil_div(p0, 64);
  int rc;
  if (p0 > 0) {
    if ((rc = s.smask.ensure((size_t)ng * 8)) || (rc = s.sbase.ensure(((size_t)ng + 1) * 8))) return rc;
    CM_HIP(hipMemsetAsync(s.sbase.as<int64_t>() + ng, 0, 8, st));
    h->timer.begin(st);
    hipLaunchKernelGGL(bm25_rm_flag_kernel, dim3((unsigned)ceil_div(p0, kRmChunk)), dim3(kRmThreads), 0, st,
                       h->post_doc.as<int32_t>(), p0, keep, s.smask.as<unsigned long long>(), s.sbase.as<int64_t>());
    CM_HIP(hipGetLastError());
    if ((rc = bm25_exclusive_sum(cub_tmp, s.sbase.as<int64_t>(), s.sbase.as<int64_t>(), ng + 1, st))) return rc;
    h->timer.end(st);
    CM_HIP(hipMemcpyAsync(&s.n, s.sbase.as<int64_t>() + ng, 8, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  return CM_OK;
}

struct FreshArrays {  // what a mutation writes; after bm25_install, the handle's old arrays (freed with it)
  TmpBuf off, doc, tf, pos, dl, live;
};

int bm25_fresh_alloc(FreshArrays &f, int32_t vocab, int64_t npost, int64_t ndocs) {
  const size_t p = (size_t)std::max<int64_t>(npost, 1), w = (size_t)std::max<int64_t>(1, ceil_div(ndocs, 32));
  int rc;
  if ((rc = f.off.ensure(((size_t)vocab + 1) * 8)) || (rc = f.doc.ensure(p * 4)) || (rc = f.tf.ensure(p * 2)) ||
      (rc = f.pos.ensure(p * 4)) || (rc = f.dl.ensure((size_t)ndocs * 4)) || (rc = f.live.ensure(w * 4)))
    return rc;
  return CM_OK;
}

// f.off from the handle's offsets (step 2 above); `s` and `d_off` may be NULL
int bm25_fresh_offsets(cm_bm25 *h, FreshArrays &f, int32_t vocab, const Survivors *s, const int64_t *d_off,
                       hipStream_t st) {
  hipLaunchKernelGGL(bm25_mut_offsets_kernel, dim3((unsigned)ceil_div((int64_t)vocab + 1, 256)), dim3(256), 0, st,
                     h->term_off.as<int64_t>(), h->vocab, vocab, h->npost, s ? s->n : 0, s ? s->mask() : nullptr,
                     s ? s->base() : nullptr, d_off, f.off.as<int64_t>());
  CM_HIP(hipGetLastError());
  return CM_OK;
}

// The one place where a mutation changes the handle: nothing of it changes before this call, so an
// error on the way leaves the index as it was.  Waits for the fresh arrays (written on `st`), swaps
// them in, sets the counts -- the index's own statistics move by (d_live, d_len), and installed ones
// give way to them, as after a build -- keeps the filtered searches' log table long enough, and
// recomputes df, the idf table and the head tiles as a build does.
int bm25_install(cm_bm25 *h, FreshArrays &f, int64_t ndocs, int64_t npost, int32_t vocab, int64_t d_live,
                 int64_t d_len, hipStream_t st) {
  CM_HIP(hipStreamSynchronize(st));
  swap_buf(h->term_off, f.off);
  swap_buf(h->post_doc, f.doc);
  swap_buf(h->post_tf, f.tf);
  swap_buf(h->post_pos, f.pos);
  swap_buf(h->dl, f.dl);
  swap_buf(h->live, f.live);
  h->ndocs = ndocs;
  h->npost = npost;
  h->vocab = vocab;
  h->n_live = h->own_live += d_live;
  h->sum_len = h->own_len += d_len;
  int rc;
  if (h->log_n >= 0 && (rc = bm25_grow_logtab(h, ndocs))) return rc;
  return bm25_finish_build(h, st);
}

// The host forms' token arrays: doc_off non-decreasing over ndocs documents, term_ids there when
// there are tokens, every id in [0, vocab).  The token count, or -1 with the error set (CM_EINVAL).
int64_t bm25_checked_ntok(const int32_t *term_ids, const int64_t *doc_off, int64_t ndocs, int32_t vocab) {
  for (int64_t d = 0; d < ndocs; ++d)
    if (doc_off[d + 1] < doc_off[d]) CM_FAIL(-1, "doc_off must be non-decreasing");
  const int64_t ntok = ndocs ? doc_off[ndocs] : 0;
  if (ntok > 0 && !term_ids) CM_FAIL(-1, "term_ids is NULL");
  for (int64_t p = 0; p < ntok; ++p)
    if (term_ids[p] < 0 || term_ids[p] >= vocab) CM_FAIL(-1, "term id out of range");
  return ntok;
}

// The host forms' rows as a bitmap of ceil(ndocs / 32) words
int bm25_rows_to_bits(const int64_t *rows, int64_t n_rows, int64_t ndocs, bool reject_duplicates,
                      std::vector<uint32_t> &bits) {
  bits.assign((size_t)ceil_div(ndocs, 32), 0u);
  for (int64_t i = 0; i < n_rows; ++i) {
    if (rows[i] < 0 || rows[i] >= ndocs) CM_FAIL(CM_EINVAL, "row out of range");
    uint32_t &w = bits[(size_t)(rows[i] >> 5)];
    if (reject_duplicates && (w & (1u << (rows[i] & 31)))) CM_FAIL(CM_EINVAL, "duplicate row");
    w |= 1u << (rows[i] & 31);
  }
  return CM_OK;
}

}  // namespace
