// cm_bm25_replace / cm_bm25_replace_dev: documents replaced in place without a rebuild (included by
// cm_bm25.hip, after cm_bm25_remove.inc, whose keep-word kernel it reuses).
//
// A replaced document keeps its row, so no row is renumbered: the new CSR is the old one without
// the replaced rows' postings, merged term by term with the delta CSR of the replacement texts.
//   delta   K7's first half (bm25_csr_from_tokens, doc_base 0) over the replacement documents:
//           d_doc holds the document's index i; rows[] is ascending, so i -> rows[i] keeps every
//           term's delta run in row order.
//   pass A  the removal's keep words (~R, R = bitmap of the replaced rows) and its flag pass with
//           the library scan: smask[] / sbase[] give surv(p), the number of surviving old postings
//           before old posting p, in O(1); surv(npost) = p_surv.
//   offsets term_off'[t] = surv(term_off[min(t, V_old)]) + d_off[t].
//   pass B  two scatters, each output slot computed from its input element alone:
//             old survivor p of term t, document d  ->  surv(p) + d_off[t] + lb,
//               lb = the delta postings of t whose row is below d;
//             delta posting j of term t, row d       ->  j + surv(p*),
//               p* = the first old posting of t whose document is >= d.
//           Within term t the survivors keep their order and so do the delta postings, a survivor
//           is never a replaced row (no ties), and slot - term_off'[t] is "survivors of t before
//           me + delta postings of t before me" for either kind: the two kernels write every slot
//           of [0, p_surv + dp) exactly once.  No merge path, no look-back between workgroups.
//   rows    dl' = dl with d_dl[i] at rows[i]; live' = live | R.
// Pass A, the offsets and the steps around them are the plan all three mutations share:
// cm_bm25_mutate.inc.
//
// Peak device memory: old + new postings (10 B each), 16 B per 64 postings (smask, sbase), the
// delta and its sort scratch.

namespace cm {

// rows[] strictly ascending and inside [0, ndocs)?  bad |= 1 otherwise.  With `bits` (zeroed by
// the caller), the valid rows' bits are set on the way (the _dev form's bitmap R).
__global__ void bm25_rp_rows_check_kernel(const int64_t *__restrict__ rows, int64_t n_rows, int64_t ndocs,
                                          uint32_t *__restrict__ bits, int32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t r = rows[i];
  if (r < 0 || r >= ndocs) {
    atomicOr(bad, 1);
    return;
  }
  if (i > 0 && rows[i - 1] >= r) atomicOr(bad, 1);
  if (bits) atomicOr(&bits[r >> 5], 1u << (r & 31));
}

// first j in [a, b) with rows[d_doc[j]] >= d (b when none): the delta postings of one term before row d
__device__ inline int64_t bm25_rp_delta_lb(const int32_t *__restrict__ d_doc, const int64_t *__restrict__ rows,
                                           int64_t a, int64_t b, int32_t d) {
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if (rows[d_doc[m]] < (int64_t)d)
      a = m + 1;
    else
      b = m;
  }
  return a;
}

// Pass B, old postings: the removal's division (one wave per 64 consecutive postings, kRmGroups
// groups per wave, kRmChunk postings per workgroup; needs npost > 0, hence v_old > 0).  The
// workgroup finds the terms of its first and last posting (block-uniform, as the append's merge),
// a lane its own between them.  A group inside one term asks for the lower bound of its first and
// last document: when they agree the whole wave shares it, otherwise a lane searches between them.
__global__ void __launch_bounds__(kRmThreads) bm25_rp_scatter_old_kernel(
    const int64_t *__restrict__ old_off, int32_t v_old, const int32_t *__restrict__ old_doc,
    const uint16_t *__restrict__ old_tf, const uint32_t *__restrict__ old_pos, int64_t npost,
    const unsigned long long *__restrict__ smask, const int64_t *__restrict__ sbase,
    const int64_t *__restrict__ d_off, const int32_t *__restrict__ d_doc, const int64_t *__restrict__ rows,
    int32_t *__restrict__ out_doc, uint16_t *__restrict__ out_tf, uint32_t *__restrict__ out_pos) {
  const int lane = threadIdx.x & 63;
  const int64_t lo = (int64_t)blockIdx.x * kRmChunk;
  if (lo >= npost) return;
  const int64_t hi = lo + kRmChunk < npost ? lo + kRmChunk : npost;
  const int32_t t_lo = bm25_term_at(old_off, 0, v_old - 1, lo);
  const int32_t t_hi = bm25_term_at(old_off, t_lo, v_old - 1, hi - 1);
  const int64_t g0 = ((int64_t)blockIdx.x * (kRmThreads / 64) + (threadIdx.x >> 6)) * kRmGroups;
  for (int u = 0; u < kRmGroups; ++u) {
    const int64_t g = g0 + u, p = g * 64 + lane;  // (g is wave-uniform)
    if (g * 64 >= npost) break;
    const unsigned long long m = smask[g];  // (bits of postings at or beyond npost are clear)
    if (!m) continue;
    const int64_t p_last = g * 64 + 63 < npost ? g * 64 + 63 : npost - 1;
    const int32_t t_first = bm25_term_at(old_off, t_lo, t_hi, g * 64);
    const int32_t t_last = bm25_term_at(old_off, t_first, t_hi, p_last);
    const bool mine = (m >> lane) & 1ull;
    const int32_t d = mine ? old_doc[p] : 0;
    int32_t t = t_first;
    int64_t a = 0, b = 0;  // the lane's delta run, narrowed where the group allows
    if (t_first == t_last) {
      a = d_off[t_first];
      b = d_off[t_first + 1];
      if (a < b) {
        const int64_t lb_first = bm25_rp_delta_lb(d_doc, rows, a, b, old_doc[g * 64]);
        const int64_t lb_last = bm25_rp_delta_lb(d_doc, rows, lb_first, b, old_doc[p_last]);
        a = lb_first;
        b = lb_last;  // (every document of the group lies between the two: so does its bound)
      }
    } else if (mine) {
      t = bm25_term_at(old_off, t_first, t_last, p);
      a = d_off[t];
      b = d_off[t + 1];
    }
    if (mine) {
      // d_off[t] + lb as one index into the delta: a is d_off[t] or beyond it by the bounds found above
      const int64_t lb = a < b ? bm25_rp_delta_lb(d_doc, rows, a, b, d) : a;
      const int64_t q = sbase[g] + (int64_t)__popcll(m & ((1ull << lane) - 1ull)) + lb;
      out_doc[q] = d;
      out_tf[q] = old_tf[p];
      out_pos[q] = old_pos[p];
    }
  }
}

// Pass B, delta postings: one thread each.  The workgroup's first and last term are block-uniform.
__global__ void __launch_bounds__(256) bm25_rp_scatter_delta_kernel(
    const int64_t *__restrict__ d_off, int32_t v_new, const int32_t *__restrict__ d_doc,
    const uint16_t *__restrict__ d_tf, const uint32_t *__restrict__ d_pos, int64_t dp,
    const int64_t *__restrict__ rows, const int64_t *__restrict__ old_off, int32_t v_old,
    const int32_t *__restrict__ old_doc, int64_t npost, const unsigned long long *__restrict__ smask,
    const int64_t *__restrict__ sbase, int64_t p_surv, int32_t *__restrict__ out_doc,
    uint16_t *__restrict__ out_tf, uint32_t *__restrict__ out_pos) {
  const int64_t lo = (int64_t)blockIdx.x * 256;
  if (lo >= dp) return;
  const int64_t hi = lo + 256 < dp ? lo + 256 : dp;
  const int32_t t_lo = bm25_term_at(d_off, 0, v_new - 1, lo);
  const int32_t t_hi = bm25_term_at(d_off, t_lo, v_new - 1, hi - 1);
  const int64_t j = lo + threadIdx.x;
  if (j >= hi) return;
  const int32_t t = bm25_term_at(d_off, t_lo, t_hi, j);
  const int32_t d = (int32_t)rows[d_doc[j]];
  int64_t a = old_off[t < v_old ? t : v_old], b = old_off[t + 1 < v_old ? t + 1 : v_old];  // (empty for t >= v_old)
  while (a < b) {  // p*: the first old posting of t at or behind row d (the replaced row's own included)
    const int64_t mid = a + (b - a) / 2;
    if (old_doc[mid] < d)
      a = mid + 1;
    else
      b = mid;
  }
  const int64_t q = j + bm25_surv(a, npost, p_surv, smask, sbase);
  out_doc[q] = d;
  out_tf[q] = d_tf[j];
  out_pos[q] = d_pos[j];
}

// dl'[rows[i]] = d_dl[i] (out_dl holds the old lengths)
__global__ void bm25_rp_dl_kernel(const int64_t *__restrict__ rows, const int32_t *__restrict__ d_dl, int64_t n_rows,
                                  int32_t *__restrict__ out_dl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_rows) out_dl[rows[i]] = d_dl[i];
}

// live' = live | R
__global__ void bm25_rp_live_kernel(const uint32_t *__restrict__ live, const uint32_t *__restrict__ repl, int64_t nw,
                                    uint32_t *__restrict__ out_live) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < nw) out_live[w] = live[w] | repl[w];
}

}  // namespace cm

namespace {

// The shared device path: n_rows > 0 rows (ascending, distinct, in range: checked by the caller)
// with their bitmap, the replacement documents' tokens, all readable on `st`; h->ndocs > 0.
int bm25_replace_device(cm_bm25 *h, const int64_t *rows_dev, const uint32_t *repl_bits_dev, int64_t n_rows,
                        const int32_t *term_ids_dev, const int64_t *doc_off_dev, int64_t ntokens, int32_t vocab,
                        hipStream_t st) {
  const int64_t n0 = h->ndocs, p0 = h->npost, nw = ceil_div(n0, 32);
  const int32_t v0 = h->vocab;
  int rc;
  CM_HIP(hipStreamSynchronize(h->stream));  // earlier work on the handle's stream read the old arrays
  // -- the delta CSR (a bad term id or offset, a tf above 65535: reported from here)
  TmpBuf d_off, d_doc, d_tf, d_pos, d_dl;
  int64_t dp = 0;
  if ((rc = bm25_csr_from_tokens(st, term_ids_dev, doc_off_dev, n_rows, ntokens, vocab, 0, d_off, d_doc, d_tf, d_pos,
                                 d_dl, &dp)))
    return rc;
  // -- keep words; the replaced rows that were live, and their lengths
  TmpBuf keep, cnt, tot, cub_tmp;
  if ((rc = keep.ensure((size_t)nw * 4)) || (rc = cnt.ensure((size_t)nw * 4)) || (rc = tot.ensure(16))) return rc;
  CM_HIP(hipMemsetAsync(tot.ptr, 0, 16, st));
  hipLaunchKernelGGL(bm25_rm_keep_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, st, repl_bits_dev,
                     h->live.as<uint32_t>(), h->dl.as<int32_t>(), n0, nw, keep.as<uint32_t>(), cnt.as<int32_t>(),
                     tot.as<unsigned long long>());
  CM_HIP(hipGetLastError());
  int64_t gone[2] = {0, 0};  // replaced rows that were live, their lengths
  CM_HIP(hipMemcpyAsync(gone, tot.ptr, 16, hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  // -- pass A and the scan: which old postings survive, and how many before each group of 64
  // (cm_bm25_timing: pass A with its scan, then the two scatters, one pair each)
  Survivors s;
  if ((rc = bm25_survivor_pass(h, keep.as<uint32_t>(), cub_tmp, s, st))) return rc;
  const int64_t p_surv = s.n, p1 = p_surv + dp;
  FreshArrays f;
  if ((rc = bm25_fresh_alloc(f, vocab, p1, n0)) || (rc = bm25_fresh_offsets(h, f, vocab, &s, d_off.as<int64_t>(), st)))
    return rc;
  if (p1 > 0) {
    h->timer.begin(st);
    if (p_surv > 0) {
      hipLaunchKernelGGL(bm25_rp_scatter_old_kernel, dim3((unsigned)ceil_div(p0, kRmChunk)), dim3(kRmThreads), 0, st,
                         h->term_off.as<int64_t>(), v0, h->post_doc.as<int32_t>(), h->post_tf.as<uint16_t>(),
                         h->post_pos.as<uint32_t>(), p0, s.mask(), s.base(), d_off.as<int64_t>(), d_doc.as<int32_t>(),
                         rows_dev, f.doc.as<int32_t>(), f.tf.as<uint16_t>(), f.pos.as<uint32_t>());
      CM_HIP(hipGetLastError());
    }
    if (dp > 0) {
      hipLaunchKernelGGL(bm25_rp_scatter_delta_kernel, dim3((unsigned)ceil_div(dp, 256)), dim3(256), 0, st,
                         d_off.as<int64_t>(), vocab, d_doc.as<int32_t>(), d_tf.as<uint16_t>(), d_pos.as<uint32_t>(),
                         dp, rows_dev, h->term_off.as<int64_t>(), v0, h->post_doc.as<int32_t>(), p0,
                         s.mask(), s.base(), p_surv, f.doc.as<int32_t>(), f.tf.as<uint16_t>(),
                         f.pos.as<uint32_t>());
      CM_HIP(hipGetLastError());
    }
    h->timer.end(st);
  }
  CM_HIP(hipMemcpyAsync(f.dl.ptr, h->dl.ptr, (size_t)n0 * 4, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(bm25_rp_dl_kernel, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, st, rows_dev,
                     d_dl.as<int32_t>(), n_rows, f.dl.as<int32_t>());
  CM_HIP(hipGetLastError());
  hipLaunchKernelGGL(bm25_rp_live_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, st, h->live.as<uint32_t>(),
                     repl_bits_dev, nw, f.live.as<uint32_t>());
  CM_HIP(hipGetLastError());
  return bm25_install(h, f, n0, p1, vocab, n_rows - gone[0], ntokens - gone[1], st);
}

// the checks both forms share; *done: nothing (more) to do, return rc
int bm25_replace_checks(cm_bm25 *h, int64_t n_rows, int32_t vocab, bool *done) {
  *done = true;
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (n_rows < 0) CM_FAIL(CM_EINVAL, "n_rows must be >= 0");
  if (n_rows == 0) return CM_OK;
  if (n_rows > h->ndocs) CM_FAIL(CM_EINVAL, "more rows than documents");
  if (vocab < h->vocab || vocab <= 0) CM_FAIL(CM_EINVAL, "vocab is below the index's");
  *done = false;
  return CM_OK;
}

}  // namespace

extern "C" {

int cm_bm25_replace_dev(cm_bm25 *h, const int64_t *rows_dev, int64_t n_rows, const int32_t *term_ids_dev,
                        const int64_t *doc_off_dev, int64_t ntokens, int32_t vocab, void *stream) {
  bool done;
  int rc = bm25_replace_checks(h, n_rows, vocab, &done);
  if (done) return rc;
  if (ntokens < 0 || !rows_dev || !doc_off_dev || (ntokens > 0 && !term_ids_dev)) CM_FAIL(CM_EINVAL, "bad arguments");
  DeviceGuard dg(h->dev);
  hipStream_t st = (hipStream_t)stream;
  // rows_dev strictly ascending and in range, read back before anything else; the bitmap on the way
  const int64_t nw = ceil_div(h->ndocs, 32);
  TmpBuf bits, bad;
  if ((rc = bits.ensure((size_t)nw * 4)) || (rc = bad.ensure(4))) return rc;
  CM_HIP(hipMemsetAsync(bits.ptr, 0, (size_t)nw * 4, st));
  CM_HIP(hipMemsetAsync(bad.ptr, 0, 4, st));
  hipLaunchKernelGGL(bm25_rp_rows_check_kernel, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, st, rows_dev,
                     n_rows, h->ndocs, bits.as<uint32_t>(), bad.as<int32_t>());
  CM_HIP(hipGetLastError());
  int32_t hbad = 0;
  CM_HIP(hipMemcpyAsync(&hbad, bad.ptr, 4, hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  if (hbad) CM_FAIL(CM_EINVAL, "rows_dev must be strictly ascending and within [0, ndocs)");
  return bm25_replace_device(h, rows_dev, bits.as<uint32_t>(), n_rows, term_ids_dev, doc_off_dev, ntokens, vocab, st);
}

int cm_bm25_replace(cm_bm25 *h, const int64_t *rows, int64_t n_rows, const int32_t *term_ids, const int64_t *doc_off,
                    int32_t vocab) {
  bool done;
  int rc = bm25_replace_checks(h, n_rows, vocab, &done);
  if (done) return rc;
  if (!rows) CM_FAIL(CM_EINVAL, "rows is NULL");
  if (!doc_off) CM_FAIL(CM_EINVAL, "doc_off is NULL");
  if (doc_off[0] != 0) CM_FAIL(CM_EINVAL, "doc_off must start at 0");
  const int64_t ntok = bm25_checked_ntok(term_ids, doc_off, n_rows, vocab);
  if (ntok < 0) return CM_EINVAL;
  std::vector<uint32_t> bits;
  if ((rc = bm25_rows_to_bits(rows, n_rows, h->ndocs, true, bits))) return rc;
  // the documents in row order: sorted rows, their tokens and offsets
  std::vector<int64_t> order((size_t)n_rows), srows((size_t)n_rows), soff((size_t)n_rows + 1, 0);
  for (int64_t i = 0; i < n_rows; ++i) order[(size_t)i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return rows[a] < rows[b]; });
  std::vector<int32_t> stid((size_t)ntok);
  for (int64_t i = 0; i < n_rows; ++i) {
    const int64_t s = order[(size_t)i], b = doc_off[s], e = doc_off[s + 1];
    srows[(size_t)i] = rows[s];
    std::copy(term_ids + b, term_ids + e, stid.begin() + soff[(size_t)i]);
    soff[(size_t)i + 1] = soff[(size_t)i] + (e - b);
  }
  DeviceGuard dg(h->dev);
  TmpBuf up_rows, up_bits, tids, offs;
  if ((rc = up_rows.ensure((size_t)n_rows * 8)) || (rc = up_bits.ensure(bits.size() * 4)) ||
      (rc = tids.ensure((size_t)std::max<int64_t>(ntok, 1) * 4)) || (rc = offs.ensure(((size_t)n_rows + 1) * 8)))
    return rc;
  CM_HIP(hipMemcpyAsync(up_rows.ptr, srows.data(), (size_t)n_rows * 8, hipMemcpyHostToDevice, h->stream));
  CM_HIP(hipMemcpyAsync(up_bits.ptr, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, h->stream));
  if (ntok) CM_HIP(hipMemcpyAsync(tids.ptr, stid.data(), (size_t)ntok * 4, hipMemcpyHostToDevice, h->stream));
  CM_HIP(hipMemcpyAsync(offs.ptr, soff.data(), ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, h->stream));
  return bm25_replace_device(h, up_rows.as<int64_t>(), up_bits.as<uint32_t>(), n_rows, tids.as<int32_t>(),
                             offs.as<int64_t>(), ntok, vocab, h->stream);
}

}  // extern "C"
