// BM25 row-list search (cm_bm25_search_lists; included by cm_bm25.hip): a batch whose queries carry
// different where clauses (BM25Store.search, rag/retrieval/bm25.py:175-212, called once per question
// by the reference).  cm_bm25_search answers one bitmap per call: a pass over all N/32 words for the
// candidate statistics, a walk of every query term's whole posting list for its candidate df, the
// pruned search.  A clause that allows a few thousand rows is answered here from its row list, and
// every clause of the batch at once:
//   1. lists  the allowed live rows of every filter as ascending CSR lists and, from the same
//             pass, the sum of dl over each list (cm_row_lists.h); the lengths (Nc) and length sums
//             are read back once.
//   2. df     bm25_list_df_kernel: one workgroup per (filter-term, 256 rows of the filter's list);
//             a thread looks its row up in the term (list_tf below), one atomic per wave.
//   3. idf    L[Nc - df] - L[df] from the handle's log table (cm_bm25_prepare_filtered's: glibc
//             logs, rank_bm25's bits); the filters with a negative idf take their epsilon floors from
//             one batched call, up to 32 of them a postings pass (cm_bm25_eps.inc).
//   4. score  bm25_list_score_kernel: one workgroup per (query, 256 rows of its filter's list), one
//             candidate per thread, the query's terms in query order with bm25_scatter_term_kernel's
//             operands: bm25_search_full's sums, hence the fused path's.
//   5. top-k  one segmented radix sort (hipCUB, stable) of (score_key, row) over the queries'
//             segments, whose input is in ascending row order; the first min(k, Nc) of each segment.
// Quirk Q2 is why the statistics are per filter; quirk Q1 (zero scores pad in row order) is the
// stable sort's.  No posting crosses to the host.
// cm_bm25_search_lists_dev is the same body with the results on the device (the top-k kernel writes
// the caller's tensors; the handle's stream first waits for the caller's) and with eps_io: epsilon
// floors the caller knows already take no postings pass, computed ones are handed back.

namespace cm {

constexpr int kBmListChunk = 256;   // rows of one list per workgroup (tests restate it)
constexpr int kBmListSlots = 64;    // query term descriptors staged in LDS at a time

// tf of (term, row), 0 when the row has no posting of the term.  A term that owns a head tile: the
// tile's byte (terms with a tf >= 255 own none, so the byte is the tf).  Otherwise a binary search of
// the term's postings, which ascend by row.  Both read what bm25_head_fill_kernel copied.
__device__ inline uint32_t bm_list_tf(int32_t head, int64_t lo, int64_t hi, int32_t row,
                                      const uint8_t *__restrict__ headtf, int64_t npad,
                                      const int32_t *__restrict__ post_doc, const uint16_t *__restrict__ post_tf) {
  if (head >= 0) return headtf[(int64_t)head * npad + row];
  const int64_t p = lower_bound_doc(post_doc, lo, hi, row);
  return (p < hi && post_doc[p] == row) ? (uint32_t)post_tf[p] : 0u;
}

// One work item of the df pass (filter-term ft, chunk of its filter's list) and of the score pass
// (query, chunk of its filter's list).
struct BmListItem {
  int32_t id, chunk;
};

// df[ft] += rows of the chunk that hold the term (zeroed by the caller).
__global__ void __launch_bounds__(256) bm25_list_df_kernel(
    const BmListItem *__restrict__ items, const int32_t *__restrict__ ft_filter, const int32_t *__restrict__ ft_term,
    const int32_t *__restrict__ rows, const int64_t *__restrict__ list_off, const int64_t *__restrict__ term_off,
    const int32_t *__restrict__ head_id, const uint8_t *__restrict__ headtf, int64_t npad,
    const int32_t *__restrict__ post_doc, const uint16_t *__restrict__ post_tf, unsigned long long *__restrict__ df) {
  const BmListItem it = items[blockIdx.x];
  const int32_t f = ft_filter[it.id], t = ft_term[it.id];
  const int64_t lo = list_off[f], len = list_off[f + 1] - lo;
  const int64_t e = (int64_t)it.chunk * kBmListChunk + threadIdx.x;
  bool has = false;
  if (e < len)
    has = bm_list_tf(head_id ? head_id[t] : -1, term_off[t], term_off[t + 1], rows[lo + e], headtf, npad, post_doc,
                     post_tf) > 0;
  const unsigned long long m = __ballot(has);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(df + it.id, (unsigned long long)__popcll(m));
}

// idf[ft] = L[Nc - df] - L[df] over the filter's candidates, 0 for df 0; neg[f] = 1 when one of
// filter f's is negative (it then takes the filter's epsilon, bm25_list_slots_kernel).
__global__ void bm25_list_idf_kernel(int n_ft, const int32_t *__restrict__ ft_filter,
                                     const int64_t *__restrict__ list_off, const unsigned long long *__restrict__ df,
                                     const double *__restrict__ logtab, double *__restrict__ idf,
                                     int32_t *__restrict__ neg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ft) return;
  const int32_t f = ft_filter[i];
  const int64_t nc = list_off[f + 1] - list_off[f], d = (int64_t)df[i];
  double v = 0.0;
  if (d > 0) {
    v = logtab[nc - d] - logtab[d];
    if (v < 0) neg[f] = 1;
  }
  idf[i] = v;
}

// What the score pass needs of one query term slot: the term's postings [lo, lo + n), its head
// tile (-1: none) and its idf under the query's filter (0: unknown term or outside the candidate
// vocabulary -- the slot is skipped).
struct BmListSlot {
  int64_t lo;
  int32_t n, head;
  double idf;
};

// slot_ft[i] = the filter-term of query term slot i, -1 for an unknown term.
__global__ void bm25_list_slots_kernel(int n_slots, const int32_t *__restrict__ slot_ft,
                                       const int32_t *__restrict__ ft_filter, const int32_t *__restrict__ ft_term,
                                       const double *__restrict__ idf, const double *__restrict__ eps,
                                       const int64_t *__restrict__ term_off, const int32_t *__restrict__ head_id,
                                       BmListSlot *__restrict__ slots) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  const int32_t ft = slot_ft[i];
  BmListSlot s{0, 0, -1, 0.0};
  if (ft >= 0) {
    const int32_t t = ft_term[ft];
    s.lo = term_off[t];
    s.n = (int32_t)(term_off[t + 1] - s.lo);   // a term's postings are at most ndocs < 2^31
    s.head = head_id ? head_id[t] : -1;
    s.idf = idf[ft] < 0 ? eps[ft_filter[ft]] : idf[ft];
  }
  slots[i] = s;
}

// The hot kernel.  256 threads, one candidate each; the query's term descriptors pass through LDS
// kBmListSlots at a time (block-uniform loop bounds and skips).  Per candidate: s = 0, then
// s = s + bm25_contrib(idf, tf, kd_of(dl[row], avgdl_f)) for every slot with tf > 0 in query order --
// bm25_scatter_term_kernel's operands and order.  The tf is looked up again per slot (bm_list_tf),
// never stored.  Key and row of list element e go to the query's segment at e: ascending rows.
__global__ void __launch_bounds__(256) bm25_list_score_kernel(
    const BmListItem *__restrict__ items, const int32_t *__restrict__ filter_of, const int32_t *__restrict__ seg_off,
    const int32_t *__restrict__ q_off, const BmListSlot *__restrict__ slots, const int32_t *__restrict__ rows,
    const int64_t *__restrict__ list_off, const double *__restrict__ avgdl, const int32_t *__restrict__ dl,
    const uint8_t *__restrict__ headtf, int64_t npad, const int32_t *__restrict__ post_doc,
    const uint16_t *__restrict__ post_tf, uint64_t *__restrict__ keys, int32_t *__restrict__ vals) {
  __shared__ BmListSlot s_slot[kBmListSlots];
  const BmListItem it = items[blockIdx.x];
  const int32_t f = filter_of[it.id];
  const int64_t lo = list_off[f], len = list_off[f + 1] - lo;
  const int64_t e = (int64_t)it.chunk * kBmListChunk + threadIdx.x;
  const bool active = e < len;
  const int32_t row = active ? rows[lo + e] : 0;
  const double kd = active ? kd_of(dl[row], avgdl[f]) : 1.0;
  double s = 0.0;
  const int tb = q_off[it.id], te = q_off[it.id + 1];
  for (int c0 = tb; c0 < te; c0 += kBmListSlots) {
    const int n = min(kBmListSlots, te - c0);
    __syncthreads();
    if ((int)threadIdx.x < n) s_slot[threadIdx.x] = slots[c0 + threadIdx.x];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const BmListSlot d = s_slot[j];
      if (d.idf == 0.0 || !active) continue;
      const uint32_t tf = bm_list_tf(d.head, d.lo, d.lo + d.n, row, headtf, npad, post_doc, post_tf);
      if (tf > 0) s = s + bm25_contrib(d.idf, tf, kd);
    }
  }
  if (active) {
    keys[(int64_t)seg_off[it.id] + e] = score_key(s);
    vals[(int64_t)seg_off[it.id] + e] = row;
  }
}

// out[i][j] = the j-th entry of query i's sorted segment; (0.0, -1) past its end.
__global__ void __launch_bounds__(256) bm25_list_topk_kernel(const uint64_t *__restrict__ sorted,
                                                             const int32_t *__restrict__ sorted_row,
                                                             const int32_t *__restrict__ seg_off, int nq, int k,
                                                             double *__restrict__ out_score,
                                                             int64_t *__restrict__ out_row) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)nq * k) return;
  const int i = (int)(idx / k), j = (int)(idx - (int64_t)i * k);
  const int32_t s0 = seg_off[i];
  if (j < seg_off[i + 1] - s0) {
    out_score[idx] = f64_unorder(~sorted[(int64_t)s0 + j]);
    out_row[idx] = (int64_t)sorted_row[(int64_t)s0 + j];
  } else {
    out_score[idx] = 0.0;
    out_row[idx] = -1;
  }
}

// cm_bm25_search_lists and cm_bm25_search_lists_dev: one body.  on_dev: out_score and out_row are
// device memory, and `stream` (the caller's) is waited for before the handle's stream starts.
// eps_io (nullable, host, n_filters doubles): the epsilon floors the caller knows, NaN = not known;
// a known one is used as it is, a computed one is written back.
static int bm25_search_lists_impl(const char *fn, bool on_dev, cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off,
                                  int32_t nq, int32_t k, const uint32_t *allow_bits, int32_t n_filters,
                                  const int32_t *filter_of, double *eps_io, double *out_score, int64_t *out_row,
                                  int32_t *out_n, hipStream_t stream) {
  const std::string F(fn);
  // ---- argument checks: host only, before any device call ----
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (nq < 1) CM_FAIL(CM_EINVAL, F + ": nq must be >= 1");
  if (k < 1) CM_FAIL(CM_EINVAL, F + ": k must be >= 1");
  if (n_filters < 1) CM_FAIL(CM_EINVAL, F + ": n_filters must be >= 1");
  if (!q_terms || !q_off || !allow_bits || !filter_of || !out_score || !out_row || !out_n)
    CM_FAIL(CM_EINVAL, "NULL argument");
  int rc;
  if ((rc = check_filter_of(F, filter_of, nq, n_filters))) return rc;
  if (q_off[0] < 0) CM_FAIL(CM_EINVAL, "bad q_off");
  for (int i = 0; i < nq; ++i)
    if (q_off[i + 1] < q_off[i]) CM_FAIL(CM_EINVAL, "q_off must be non-decreasing");
  DeviceGuard dg(h->dev);
  const int64_t ndocs = h->ndocs;
  const int32_t n_slots = q_off[nq];
  h->last_eps_filters = 0;
  h->last_eps_passes = 0;
  if (on_dev && (rc = stream_wait_stream(h->stream, stream))) return rc;   // the producer of allow_bits
  // ---- 1. lists: count + length sums, scan, one read-back ----
  RowLists lists;
  if ((rc = row_lists_count(F, "ndocs", allow_bits, n_filters, h->live.as<uint32_t>(), h->dl.as<int32_t>(), ndocs,
                            h->allow_buf, h->tmp, h->stream, lists)))
    return rc;
  const int64_t *off = lists.stat.data(), *sum_len = off + n_filters + 1, nw = lists.n_words;
  const int64_t n_rows = off[n_filters];
  // ---- the queries' segments (host) ----
  std::vector<int32_t> seg;
  int64_t n_keys = 0;
  for (int i = 0; i < nq; ++i) {
    const int f = filter_of[i];
    const int64_t nc = off[f + 1] - off[f];
    if (nc > 0 && sum_len[f] == 0)
      CM_FAIL(CM_EZERODIV, "float division by zero (candidate documents have no tokens)");
    out_n[i] = (int32_t)std::min<int64_t>(k, nc);
  }
  if ((rc = row_list_segments(F, off, filter_of, nq, seg, n_keys))) return rc;
  // ---- (filter, distinct known term) pairs of the queries that use the filter, and every slot's ----
  std::vector<int32_t> slot_ft((size_t)std::max(n_slots, 1), -1);
  std::vector<uint64_t> ftkey;
  for (int i = 0; i < nq; ++i) {
    if (off[filter_of[i] + 1] == off[filter_of[i]]) continue;   // nothing is scored under an empty list
    for (int32_t j = q_off[i]; j < q_off[i + 1]; ++j)
      if (q_terms[j] >= 0 && q_terms[j] < h->vocab) ftkey.push_back(((uint64_t)filter_of[i] << 32) | (uint32_t)q_terms[j]);
  }
  std::sort(ftkey.begin(), ftkey.end());
  ftkey.erase(std::unique(ftkey.begin(), ftkey.end()), ftkey.end());
  const int64_t n_ft = (int64_t)ftkey.size();
  std::vector<int32_t> ft_filter((size_t)n_ft), ft_term((size_t)n_ft);
  std::vector<BmListItem> df_items, sc_items;
  for (int64_t u = 0; u < n_ft; ++u) {
    const int32_t f = (int32_t)(ftkey[u] >> 32);
    ft_filter[u] = f;
    ft_term[u] = (int32_t)(uint32_t)ftkey[u];
    for (int64_t c = 0; c < ceil_div(off[f + 1] - off[f], kBmListChunk); ++c)
      df_items.push_back(BmListItem{(int32_t)u, (int32_t)c});
  }
  for (int i = 0; i < nq; ++i) {
    const int f = filter_of[i];
    if (off[f + 1] == off[f]) continue;
    for (int32_t j = q_off[i]; j < q_off[i + 1]; ++j)
      if (q_terms[j] >= 0 && q_terms[j] < h->vocab)
        slot_ft[j] = (int32_t)(std::lower_bound(ftkey.begin(), ftkey.end(), ((uint64_t)f << 32) | (uint32_t)q_terms[j]) -
                               ftkey.begin());
    for (int64_t c = 0; c < ceil_div(off[f + 1] - off[f], kBmListChunk); ++c)
      sc_items.push_back(BmListItem{i, (int32_t)c});
  }
  if (df_items.size() > (size_t)INT32_MAX || n_ft > INT32_MAX)
    CM_FAIL(CM_EUNSUPPORTED, F + ": too many work items: split the batch");
  std::vector<double> avgdl((size_t)n_filters, 1.0);   // (Nc == 0: nothing is scored)
  for (int f = 0; f < n_filters; ++f)
    if (off[f + 1] > off[f]) avgdl[f] = (double)sum_len[f] / (double)(off[f + 1] - off[f]);
  // ---- workspace: laid out once, now that every size is known (ensure may move the buffer) ----
  size_t sort_b = 0;
  if (n_keys > 0)
    CM_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(
        nullptr, sort_b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr,
        (int)n_keys, nq, (const int32_t *)nullptr, (const int32_t *)nullptr, 0, 64, h->stream));
  char *sort_ws;
  int32_t *rows, *ftf_dev, *ftt_dev, *neg_dev, *sft_dev, *qoff_dev, *fof_dev, *seg_dev, *vals, *svals;
  BmListItem *dfi_dev, *sci_dev;
  unsigned long long *df_dev;
  double *idf_dev, *eps_dev, *avg_dev, *osc_dev;
  BmListSlot *slots_dev;
  uint64_t *keys, *skeys;
  int64_t *orow_dev;
  const auto carve = [&](char *base) {   // the bytes it takes
    Carver c{base};
    sort_ws = c.take<char>(sort_b);
    rows = c.take<int32_t>((size_t)n_rows);
    dfi_dev = c.take<BmListItem>(df_items.size());
    sci_dev = c.take<BmListItem>(sc_items.size());
    ftf_dev = c.take<int32_t>((size_t)n_ft);
    ftt_dev = c.take<int32_t>((size_t)n_ft);
    df_dev = c.take<unsigned long long>((size_t)n_ft);
    idf_dev = c.take<double>((size_t)n_ft);
    neg_dev = c.take<int32_t>((size_t)n_filters);
    eps_dev = c.take<double>((size_t)n_filters);
    avg_dev = c.take<double>((size_t)n_filters);
    sft_dev = c.take<int32_t>((size_t)n_slots);
    slots_dev = c.take<BmListSlot>((size_t)n_slots);
    qoff_dev = c.take<int32_t>((size_t)nq + 1);
    fof_dev = c.take<int32_t>((size_t)nq);
    seg_dev = c.take<int32_t>((size_t)nq + 1);
    keys = c.take<uint64_t>((size_t)n_keys);
    skeys = c.take<uint64_t>((size_t)n_keys);
    vals = c.take<int32_t>((size_t)n_keys);
    svals = c.take<int32_t>((size_t)n_keys);
    osc_dev = c.take<double>((size_t)nq * k);
    orow_dev = c.take<int64_t>((size_t)nq * k);
    return c.off;
  };
  if ((rc = h->ws.ensure(carve(nullptr)))) return rc;
  if (n_keys > 0 && (rc = bm25_grow_logtab(h, ndocs))) return rc;
  carve(h->ws.as<char>());
  // (device form: the top-k kernel writes the caller's tensors)
  double *d_score = on_dev ? out_score : osc_dev;
  int64_t *d_row = on_dev ? out_row : orow_dev;
  const int32_t *head_id = h->nhead ? h->head_id.as<int32_t>() : (const int32_t *)nullptr;
  std::vector<double> eps((size_t)n_filters, 0.0);   // (host sources of async copies: alive until the last synchronise)
  CM_HIP(hipMemcpyAsync(seg_dev, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, h->stream));
  if (n_keys > 0) {
    CM_HIP(hipMemcpyAsync(qoff_dev, q_off, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, h->stream));
    CM_HIP(hipMemcpyAsync(fof_dev, filter_of, (size_t)nq * 4, hipMemcpyHostToDevice, h->stream));
    CM_HIP(hipMemcpyAsync(avg_dev, avgdl.data(), avgdl.size() * 8, hipMemcpyHostToDevice, h->stream));
    CM_HIP(hipMemcpyAsync(sci_dev, sc_items.data(), sc_items.size() * 8, hipMemcpyHostToDevice, h->stream));
    if (n_slots > 0) CM_HIP(hipMemcpyAsync(sft_dev, slot_ft.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, h->stream));
    // ---- 1b. the lists ----
    if ((rc = row_lists_scatter(lists, h->live.as<uint32_t>(), ndocs, rows, h->stream))) return rc;
    if (n_ft > 0) {
      // ---- 2. candidate df ----
      CM_HIP(hipMemcpyAsync(ftf_dev, ft_filter.data(), (size_t)n_ft * 4, hipMemcpyHostToDevice, h->stream));
      CM_HIP(hipMemcpyAsync(ftt_dev, ft_term.data(), (size_t)n_ft * 4, hipMemcpyHostToDevice, h->stream));
      CM_HIP(hipMemcpyAsync(dfi_dev, df_items.data(), df_items.size() * 8, hipMemcpyHostToDevice, h->stream));
      CM_HIP(hipMemsetAsync(df_dev, 0, (size_t)n_ft * 8, h->stream));
      CM_HIP(hipMemsetAsync(neg_dev, 0, (size_t)n_filters * 4, h->stream));
      hipLaunchKernelGGL(bm25_list_df_kernel, dim3((unsigned)df_items.size()), dim3(256), 0, h->stream, dfi_dev, ftf_dev,
                         ftt_dev, rows, lists.off_dev, h->term_off.as<int64_t>(), head_id, h->headtf.as<uint8_t>(), h->npad,
                         h->post_doc.as<int32_t>(), h->post_tf.as<uint16_t>(), df_dev);
      CM_HIP(hipGetLastError());
      // ---- 3. idf, and the epsilon of the filters that have a negative one ----
      hipLaunchKernelGGL(bm25_list_idf_kernel, dim3((unsigned)ceil_div(n_ft, 256)), dim3(256), 0, h->stream, (int)n_ft,
                         ftf_dev, lists.off_dev, df_dev, h->logtab.as<double>(), idf_dev, neg_dev);
      CM_HIP(hipGetLastError());
      std::vector<int32_t> neg((size_t)n_filters, 0);
      CM_HIP(hipMemcpyAsync(neg.data(), neg_dev, neg.size() * 4, hipMemcpyDeviceToHost, h->stream));
      CM_HIP(hipStreamSynchronize(h->stream));
      std::vector<int64_t> e_off, e_nc, e_len;   // the filters with a negative idf: one batched call (cm_bm25_eps.inc)
      std::vector<int32_t> e_f;
      bool any_neg = false;
      for (int f = 0; f < n_filters; ++f) {
        if (!neg[f]) continue;
        any_neg = true;
        if (eps_io && !std::isnan(eps_io[f])) {   // the caller's floor: no postings pass for this filter
          eps[f] = eps_io[f];
          continue;
        }
        e_f.push_back(f);
        e_off.push_back((int64_t)f * nw);
        e_nc.push_back(off[f + 1] - off[f]);
        e_len.push_back(sum_len[f]);
      }
      if (!e_f.empty()) {
        // (reads the filters' bitmaps where they lie; writes eps_ws only)
        std::vector<double> e_eps(e_f.size(), 0.0);
        if ((rc = bm25_eps_multi(h, h->allow_buf.as<uint32_t>(), (int)e_f.size(), e_off.data(), e_nc.data(), e_len.data(),
                                 e_eps.data())))
          return rc;
        for (size_t u = 0; u < e_f.size(); ++u) {
          eps[e_f[u]] = e_eps[u];
          if (eps_io) eps_io[e_f[u]] = e_eps[u];
        }
        h->last_eps_filters = (int32_t)e_f.size();
      }
      if (any_neg) CM_HIP(hipMemcpyAsync(eps_dev, eps.data(), eps.size() * 8, hipMemcpyHostToDevice, h->stream));
    }
    if (n_slots > 0) {
      hipLaunchKernelGGL(bm25_list_slots_kernel, dim3((unsigned)ceil_div(n_slots, 256)), dim3(256), 0, h->stream,
                         (int)n_slots, sft_dev, ftf_dev, ftt_dev, idf_dev, eps_dev, h->term_off.as<int64_t>(), head_id,
                         slots_dev);
      CM_HIP(hipGetLastError());
    }
    // ---- 4. scores ----
    h->timer.begin(h->stream);
    hipLaunchKernelGGL(bm25_list_score_kernel, dim3((unsigned)sc_items.size()), dim3(256), 0, h->stream, sci_dev, fof_dev,
                       seg_dev, qoff_dev, slots_dev, rows, lists.off_dev, avg_dev, h->dl.as<int32_t>(), h->headtf.as<uint8_t>(),
                       h->npad, h->post_doc.as<int32_t>(), h->post_tf.as<uint16_t>(), keys, vals);
    CM_HIP(hipGetLastError());
    h->timer.end(h->stream);
    // ---- 5. top-k ----
    CM_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(sort_ws, sort_b, keys, skeys, vals, svals, (int)n_keys, nq,
                                                       seg_dev, seg_dev + 1, 0, 64, h->stream));
  }
  hipLaunchKernelGGL(bm25_list_topk_kernel, dim3((unsigned)ceil_div((int64_t)nq * k, 256)), dim3(256), 0, h->stream,
                     skeys, svals, seg_dev, nq, k, d_score, d_row);
  CM_HIP(hipGetLastError());
  if (!on_dev) {
    CM_HIP(hipMemcpyAsync(out_score, d_score, (size_t)nq * k * 8, hipMemcpyDeviceToHost, h->stream));
    CM_HIP(hipMemcpyAsync(out_row, d_row, (size_t)nq * k * 8, hipMemcpyDeviceToHost, h->stream));
  }
  CM_HIP(hipStreamSynchronize(h->stream));   // the host sources above, and the outputs: complete on return
  h->last_rescored = -1;
  return CM_OK;
}

}  // namespace cm

extern "C" {

int cm_bm25_search_lists(cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off, int32_t nq, int32_t k,
                         const uint32_t *allow_bits, int32_t n_filters, const int32_t *filter_of, double *out_score,
                         int64_t *out_row, int32_t *out_n) {
  return bm25_search_lists_impl("cm_bm25_search_lists", false, h, q_terms, q_off, nq, k, allow_bits, n_filters,
                                filter_of, nullptr, out_score, out_row, out_n, nullptr);
}

int cm_bm25_search_lists_dev(cm_bm25 *h, const int32_t *q_terms, const int32_t *q_off, int32_t nq, int32_t k,
                             const uint32_t *allow_bits, int32_t n_filters, const int32_t *filter_of, double *eps_io,
                             double *score_dev, int64_t *row_dev, int32_t *out_n, void *stream) {
  return bm25_search_lists_impl("cm_bm25_search_lists_dev", true, h, q_terms, q_off, nq, k, allow_bits, n_filters,
                                filter_of, eps_io, score_dev, row_dev, out_n, static_cast<hipStream_t>(stream));
}

int32_t cm_bm25_last_eps_filters(cm_bm25 *h) { return h ? h->last_eps_filters : -1; }

}  // extern "C"
