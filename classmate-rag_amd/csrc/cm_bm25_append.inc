// cm_bm25_append / cm_bm25_append_dev: new documents without a rebuild (included by cm_bm25.hip).
//
// The new documents take the rows after the existing ones, so every term's new postings follow
// its old ones.  K7's first half (bm25_csr_from_tokens) turns the new tokens into a delta CSR in
// scratch; the offsets add up (term_off'[t] = term_off[min(t, V_old)] + delta_off[t]) and one kernel
// streams both posting sets into fresh arrays, each term's old run followed by its delta run.  The
// steps around that are the plan all three mutations share: cm_bm25_mutate.inc.
//
// Peak device memory: old + new postings (10 B each) plus the delta's sort scratch; the old arrays
// are freed when the call returns.

namespace cm {

constexpr int kAppThreads = 256;
constexpr int kAppGroups = 4;  // groups of 4 consecutive postings per thread
constexpr int64_t kAppChunk = (int64_t)kAppThreads * 4 * kAppGroups;  // output postings per workgroup

struct AppTerm {  // where term t's postings lie: [begin, end) merged = n_old old ones from src_old, then the delta's
  int64_t begin, end, src_old, n_old, src_delta;
};
__device__ inline AppTerm bm25_app_term(int32_t t, const int64_t *__restrict__ new_off,
                                        const int64_t *__restrict__ old_off, const int64_t *__restrict__ delta_off,
                                        int32_t v_old) {
  AppTerm a;
  a.begin = new_off[t];
  a.end = new_off[t + 1];
  a.src_old = old_off[t < v_old ? t : v_old];
  a.n_old = old_off[t + 1 < v_old ? t + 1 : v_old] - a.src_old;
  a.src_delta = delta_off[t];
  return a;
}

// The merge is divided by output postings, not by terms (one head term of a Zipfian corpus owns
// millions of postings): workgroup b writes out[b kAppChunk, (b + 1) kAppChunk).  It finds the
// terms of its first and last posting by binary search in new_off (block-uniform: scalar loads);
// a thread then takes 4 consecutive postings at a time (16-byte stores), finds the first one's term
// between those two and moves forward from it -- inside a head term no search step is left.
__global__ void __launch_bounds__(kAppThreads) bm25_append_merge_kernel(
    const int64_t *__restrict__ new_off, const int64_t *__restrict__ old_off, const int64_t *__restrict__ delta_off,
    int32_t v_old, int32_t v_new, int64_t npost, const int32_t *__restrict__ old_doc,
    const uint16_t *__restrict__ old_tf, const uint32_t *__restrict__ old_pos, const int32_t *__restrict__ d_doc,
    const uint16_t *__restrict__ d_tf, const uint32_t *__restrict__ d_pos, int32_t *__restrict__ out_doc,
    uint16_t *__restrict__ out_tf, uint32_t *__restrict__ out_pos) {
  const int64_t lo = (int64_t)blockIdx.x * kAppChunk;
  const int64_t hi = lo + kAppChunk < npost ? lo + kAppChunk : npost;
  if (lo >= hi) return;
  const int32_t t_lo = bm25_term_at(new_off, 0, v_new - 1, lo);
  const int32_t t_hi = bm25_term_at(new_off, t_lo, v_new - 1, hi - 1);
  for (int g = 0; g < kAppGroups; ++g) {
    const int64_t q = lo + ((int64_t)g * kAppThreads + threadIdx.x) * 4;
    if (q >= hi) break;
    int32_t t = bm25_term_at(new_off, t_lo, t_hi, q);
    AppTerm a = bm25_app_term(t, new_off, old_off, delta_off, v_old);
    int32_t doc[4] = {0, 0, 0, 0};
    uint32_t pos[4] = {0, 0, 0, 0};
    uint16_t tf[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t p = q + j;
      if (p < hi) {
        if (p >= a.end) {  // the next term with a posting (empty terms in between are skipped)
          t = bm25_term_at(new_off, t + 1, t_hi, p);
          a = bm25_app_term(t, new_off, old_off, delta_off, v_old);
        }
        const int64_t r = p - a.begin;
        if (r < a.n_old) {
          const int64_t s = a.src_old + r;
          doc[j] = old_doc[s];
          tf[j] = old_tf[s];
          pos[j] = old_pos[s];
        } else {
          const int64_t s = a.src_delta + (r - a.n_old);
          doc[j] = d_doc[s];
          tf[j] = d_tf[s];
          pos[j] = d_pos[s];
        }
      }
    }
    if (q + 4 <= hi) {  // q is a multiple of 4 and the arrays are hipMalloc'ed: aligned
      *reinterpret_cast<int4 *>(out_doc + q) = make_int4(doc[0], doc[1], doc[2], doc[3]);
      *reinterpret_cast<ushort4 *>(out_tf + q) = make_ushort4(tf[0], tf[1], tf[2], tf[3]);
      *reinterpret_cast<uint4 *>(out_pos + q) = make_uint4(pos[0], pos[1], pos[2], pos[3]);
    } else {
      for (int j = 0; q + j < hi; ++j) {
        out_doc[q + j] = doc[j];
        out_tf[q + j] = tf[j];
        out_pos[q + j] = pos[j];
      }
    }
  }
}

// live bits of rows [n_old, n_new) set; the rows before keep theirs (a partial last word included).
// bits[] holds the old words in front; one thread per word from n_old / 32 on.
__global__ void bm25_append_live_kernel(uint32_t *__restrict__ bits, int64_t n_old, int64_t n_new) {
  const int64_t w = (n_old >> 5) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= n_new) return;
  const int64_t first = n_old > w * 32 ? n_old - w * 32 : 0;  // first new bit of this word
  const int64_t rem = n_new - w * 32;
  uint32_t m = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
  m &= ~((1u << first) - 1u);  // (first < 32)
  bits[w] = first ? (bits[w] | m) : m;
}

}  // namespace cm

namespace {

// The shared device path: n_new > 0 documents (device arrays on `st`) after the h->ndocs > 0
// existing ones.
int bm25_append_device(cm_bm25 *h, const int32_t *term_ids_dev, const int64_t *doc_off_dev, int64_t n_new,
                       int64_t ntokens, int32_t vocab, hipStream_t st) {
  const int64_t n0 = h->ndocs, n1 = n0 + n_new, p0 = h->npost;
  const int32_t v0 = h->vocab;
  int rc;
  CM_HIP(hipStreamSynchronize(h->stream));  // earlier work on the handle's stream read the old arrays
  TmpBuf d_off, d_doc, d_tf, d_pos, d_dl;
  int64_t dp = 0;
  if ((rc = bm25_csr_from_tokens(st, term_ids_dev, doc_off_dev, n_new, ntokens, vocab, n0, d_off, d_doc, d_tf, d_pos,
                                 d_dl, &dp)))
    return rc;
  const int64_t p1 = p0 + dp;
  const int64_t w0 = std::max<int64_t>(1, ceil_div(n0, 32)), w1 = ceil_div(n1, 32);
  FreshArrays f;
  if ((rc = bm25_fresh_alloc(f, vocab, p1, n1)) || (rc = bm25_fresh_offsets(h, f, vocab, nullptr, d_off.as<int64_t>(), st)))
    return rc;
  if (p1 > 0) {
    h->timer.begin(st);  // cm_bm25_timing: the merge kernel alone
    hipLaunchKernelGGL(bm25_append_merge_kernel, dim3((unsigned)ceil_div(p1, kAppChunk)), dim3(kAppThreads), 0, st,
                       f.off.as<int64_t>(), h->term_off.as<int64_t>(), d_off.as<int64_t>(), v0, vocab, p1,
                       h->post_doc.as<int32_t>(), h->post_tf.as<uint16_t>(), h->post_pos.as<uint32_t>(),
                       d_doc.as<int32_t>(), d_tf.as<uint16_t>(), d_pos.as<uint32_t>(), f.doc.as<int32_t>(),
                       f.tf.as<uint16_t>(), f.pos.as<uint32_t>());
    h->timer.end(st);
    CM_HIP(hipGetLastError());
  }
  CM_HIP(hipMemcpyAsync(f.dl.ptr, h->dl.ptr, (size_t)n0 * 4, hipMemcpyDeviceToDevice, st));
  CM_HIP(hipMemcpyAsync(f.dl.as<int32_t>() + n0, d_dl.ptr, (size_t)n_new * 4, hipMemcpyDeviceToDevice, st));
  CM_HIP(hipMemcpyAsync(f.live.ptr, h->live.ptr, (size_t)w0 * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(bm25_append_live_kernel, dim3((unsigned)ceil_div(w1 - (n0 >> 5), 256)), dim3(256), 0, st,
                     f.live.as<uint32_t>(), n0, n1);
  CM_HIP(hipGetLastError());
  return bm25_install(h, f, n1, p1, vocab, n_new, ntokens, st);
}

// the checks both forms share; *done: nothing (more) to do, return rc
int bm25_append_checks(cm_bm25 *h, int64_t n_new, int32_t vocab, bool *done) {
  *done = true;
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (n_new < 0) CM_FAIL(CM_EINVAL, "n_new must be >= 0");
  if (n_new == 0) return CM_OK;
  if (vocab < h->vocab) CM_FAIL(CM_EINVAL, "vocab is below the index's");
  if (h->ndocs + n_new >= (int64_t)INT32_MAX) CM_FAIL(CM_EINVAL, "too many docs for one shard");
  *done = false;
  return CM_OK;
}

}  // namespace

extern "C" {

int cm_bm25_append_dev(cm_bm25 *h, const int32_t *term_ids_dev, const int64_t *doc_off_dev, int64_t n_new,
                       int64_t ntokens, int32_t vocab, void *stream) {
  bool done;
  int rc = bm25_append_checks(h, n_new, vocab, &done);
  if (done) return rc;
  if (ntokens < 0 || vocab <= 0 || !doc_off_dev || (ntokens > 0 && !term_ids_dev)) CM_FAIL(CM_EINVAL, "bad arguments");
  DeviceGuard dg(h->dev);
  if (h->ndocs == 0) {  // nothing to merge with: the build
    if ((rc = cm_bm25_build_dev(h, term_ids_dev, doc_off_dev, n_new, ntokens, vocab, stream)) && rc != CM_EZERODIV)
      return rc;
    const int rc2 = h->log_n >= 0 ? bm25_grow_logtab(h, h->ndocs) : CM_OK;
    return rc2 ? rc2 : rc;
  }
  return bm25_append_device(h, term_ids_dev, doc_off_dev, n_new, ntokens, vocab, (hipStream_t)stream);
}

int cm_bm25_append(cm_bm25 *h, const int32_t *term_ids, const int64_t *doc_off, int64_t n_new, int32_t vocab) {
  bool done;
  int rc = bm25_append_checks(h, n_new, vocab, &done);
  if (done) return rc;
  if (!doc_off) CM_FAIL(CM_EINVAL, "doc_off is NULL");
  if (doc_off[0] != 0) CM_FAIL(CM_EINVAL, "doc_off must start at 0");
  const int64_t ntok = bm25_checked_ntok(term_ids, doc_off, n_new, vocab);
  if (ntok < 0) return CM_EINVAL;
  DeviceGuard dg(h->dev);
  if (h->ndocs == 0) {
    if ((rc = cm_bm25_build(h, term_ids, doc_off, n_new, vocab, nullptr)) && rc != CM_EZERODIV) return rc;
    const int rc2 = h->log_n >= 0 ? bm25_grow_logtab(h, h->ndocs) : CM_OK;
    return rc2 ? rc2 : rc;
  }
  // only the new documents' term ids and offsets go up; the rest is the device path
  TmpBuf tids, offs;
  if ((rc = tids.ensure((size_t)std::max<int64_t>(ntok, 1) * 4)) || (rc = offs.ensure(((size_t)n_new + 1) * 8)))
    return rc;
  if (ntok) CM_HIP(hipMemcpyAsync(tids.ptr, term_ids, (size_t)ntok * 4, hipMemcpyHostToDevice, h->stream));
  CM_HIP(hipMemcpyAsync(offs.ptr, doc_off, ((size_t)n_new + 1) * 8, hipMemcpyHostToDevice, h->stream));
  return bm25_append_device(h, tids.as<int32_t>(), offs.as<int64_t>(), n_new, ntok, vocab, h->stream);
}

}  // extern "C"
