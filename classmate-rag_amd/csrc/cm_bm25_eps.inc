// The epsilon floors of many filters from shared postings passes (cm_bm25_filter_eps_multi, and
// cm_bm25_search_lists' stage 3; included by cm_bm25.hip).  filtered_eps answers one filter per call:
// one workgroup per vocabulary term over all postings, two V-sized arrays to the host, a host sort of
// the candidate vocabulary, two glibc logs per term.  Here up to 32 filters share one pass, and
// nothing but a (sum, count) pair per filter crosses to the host.  Filters are taken in rounds of
// R <= 32 (bm25_eps_plan); per round, all on the handle's stream:
//   1. memb   memb[d] bit j = live & allow_j of document d, for d < ndocs (bits of a bitmap's last
//             word at or above ndocs are never read).
//   2. pass   bm25_eps_post_kernel: the postings array is cut into slices of kBmEpsSlice postings,
//             whatever the terms; a wave takes a slice and walks the terms that lie in it, 64
//             postings at a time: it gathers memb[post_doc[p]], ORs the words across the wave and
//             loops over the set bits only: a ballot and a popcount per bit for df; the lowest lane of
//             the first non-empty ballot of a (term, filter) is the first candidate posting (postings
//             ascend by document), whose post_pos is read only then.  Lane j keeps filter j's (df,
//             first) of the current term.  A term that lies inside the slice emits its tuples
//             (first, filter, df) at once; a term that crosses a slice border (at most one begins in
//             any slice) is merged in a table by atomicAdd (df) and atomicMin (first), and
//             bm25_eps_merge_kernel emits its tuples.  A filter's tuples go to its own segment,
//             sized by its bound, through a cursor from which a lane takes kBmEpsChunk slots at a
//             time; the slots nobody fills keep the key ~0 they were set to.
//   3. order  a stable radix sort of all the round's slots by `first` (doc << 32 | post_pos)...
//   4. idf    ... each sorted tuple's df becomes L[Nc - df] - L[df] (the handle's log table: glibc
//             logs, bm25_idf's bits) with its filter as an 8-bit key, unfilled slots the key 63...
//   5.        ... and a second stable sort, by those 6 bits: every filter's idfs contiguous, in
//             ascending `first`, filter j's after those of the filters before it.
//   6. sum    one wave per filter: sum = 0.0, then sum = sum + idf over its run in order, the lanes
//             loading 64 values and one chain of adds consuming them; (sum, count) out.
// The host forms 0.25 * (sum / (double)count) after the one read-back: filtered_eps' expression on
// filtered_eps' operands.
//
// This header restates no arithmetic of its own: the same two table logs and one subtraction per
// term, the same sequential fp64 adds in the same order (the keys are distinct within a filter, so
// the order is total and the sorts' stability between filters is all that is asked of them).

namespace cm {

constexpr int kBmEpsSlice = 4096;                  // postings a wave walks of one term at most (tests restate it)
constexpr int kBmEpsFilters = 32;                  // filters of one round: the bits of a membership word
constexpr int kBmEpsChunk = 8;                     // tuple slots a lane takes from a filter's cursor at a time
constexpr int kBmEpsCursorStride = 32;             // uint32 words between two cursors: a 128-B line each
constexpr int64_t kBmEpsTupleBudget = 1ll << 23;   // tuple bounds of one round, summed (8 B x 4 arrays each)

// One round, as the kernels read it.  seg[j] .. seg[j + 1]: filter j's tuple slots.
struct BmEpsRound {
  int32_t n, pad;
  int32_t out[kBmEpsFilters];         // where the filter's (sum, count) goes in the call's results
  int64_t allow_off[kBmEpsFilters];   // its bitmap's first word in the allow array
  int64_t nc[kBmEpsFilters];          // its candidates
  int64_t seg[kBmEpsFilters + 1];
};

struct BmEpsResult {
  double sum;
  int64_t count;
};

__global__ void __launch_bounds__(256) bm25_eps_memb_kernel(const uint32_t *__restrict__ allow,
                                                            const uint32_t *__restrict__ live, int64_t ndocs,
                                                            const BmEpsRound *__restrict__ r,
                                                            uint32_t *__restrict__ memb) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= ndocs) return;
  const int64_t w = d >> 5;
  const int b = (int)(d & 31);
  uint32_t m = 0;
  if ((live[w] >> b) & 1u) {
    const int n = r->n;
    for (int j = 0; j < n; ++j) m |= ((allow[r->allow_off[j] + w] >> b) & 1u) << j;
  }
  memb[d] = m;
}

// Slot for one more tuple of filter j (the calling lane's): from the lane's chunk, or a fresh chunk
// of the filter's cursor.  -1, and *overflow set, past the segment's end: the bounds make that
// impossible, and no store is ever made on the strength of that alone.
__device__ inline int64_t bm25_eps_slot(const BmEpsRound *__restrict__ r, int j, int take, uint32_t *cursor,
                                        int64_t &cur, int &left, int32_t *overflow) {
  if (left == 0) {
    cur = r->seg[j] + (int64_t)atomicAdd(cursor + j * kBmEpsCursorStride, (uint32_t)take);
    left = take;
  }
  const int64_t s = cur;
  cur += 1;
  left -= 1;
  if (s >= r->seg[j + 1]) {
    *overflow = 1;
    return -1;
  }
  return s;
}

__device__ inline uint64_t bm25_eps_val(int j, uint32_t df) { return ((uint64_t)j << 56) | df; }

__global__ void __launch_bounds__(256) bm25_eps_post_kernel(
    const int64_t *__restrict__ term_off, const int32_t *__restrict__ post_doc, const uint32_t *__restrict__ post_pos,
    int32_t vocab, int64_t npost, int64_t n_slices, int64_t ndocs, const uint32_t *__restrict__ memb,
    const BmEpsRound *__restrict__ r, uint32_t *__restrict__ cursor, uint32_t *__restrict__ nt,
    uint32_t *__restrict__ tab_df, unsigned long long *__restrict__ tab_first, uint64_t *__restrict__ keys,
    uint64_t *__restrict__ vals, int32_t *__restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  int64_t cur = 0;        // lane j < 32: filter j's chunk of slots, tuples emitted, the current term's df and first
  int left = 0;
  uint32_t emitted = 0, df = 0;
  uint64_t first = 0;
  for (int64_t s = wave; s < n_slices; s += n_waves) {
    const int64_t s0 = s * kBmEpsSlice, s1 = min(s0 + (int64_t)kBmEpsSlice, npost);
    // the first term that ends beyond s0 (wave-uniform)
    int32_t t = 0;
    for (int32_t end = vocab; t < end;) {
      const int32_t mid = t + (end - t) / 2;
      if (term_off[mid + 1] > s0) end = mid; else t = mid + 1;
    }
    for (; t < vocab; ++t) {
      const int64_t lo = term_off[t], hi = term_off[t + 1];
      if (lo >= s1) break;
      if (hi <= lo) continue;
      const int64_t a = max(lo, s0), b = min(hi, s1);
      uint32_t seen = 0;   // filters with a candidate posting of this term so far (wave-uniform)
      for (int64_t p0 = a; p0 < b; p0 += 64) {
        const int64_t p = p0 + lane;
        const int32_t d = p < b ? post_doc[p] : -1;
        const uint32_t m = d >= 0 && d < ndocs ? memb[d] : 0u;
        if (__ballot(m != 0u) == 0ull) continue;
        uint32_t any = m;
        for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o);
        any = __builtin_amdgcn_readfirstlane(any);
        while (any) {
          const int j = __ffs(any) - 1;
          any &= any - 1;
          const unsigned long long bal = __ballot((m >> j) & 1u);
          if (!((seen >> j) & 1u)) {
            seen |= 1u << j;
            const int src = __ffsll(bal) - 1;
            const uint64_t key = ((uint64_t)(uint32_t)__shfl(d, src) << 32) | post_pos[p0 + src];
            if (lane == j) first = key;
          }
          if (lane == j) df += (uint32_t)__popcll(bal);
        }
      }
      if (!seen) continue;
      if (lane < kBmEpsFilters && df > 0) {
        if (lo >= s0 && hi <= s1) {
          const int64_t slot = bm25_eps_slot(r, lane, kBmEpsChunk, cursor, cur, left, overflow);
          if (slot >= 0) {
            keys[slot] = first;
            vals[slot] = bm25_eps_val(lane, df);
            emitted += 1;
          }
        } else {   // the one term that begins in slice lo / kBmEpsSlice and crosses its end
          const int64_t e = (lo / kBmEpsSlice) * kBmEpsFilters + lane;
          atomicAdd(tab_df + e, df);
          atomicMin(tab_first + e, (unsigned long long)first);
        }
      }
      df = 0;
    }
  }
  if (lane < kBmEpsFilters && emitted) atomicAdd(nt + lane, emitted);
}

// The tuples of the terms that crossed a slice border: entry e = (slice the term begins in, filter).
__global__ void __launch_bounds__(256) bm25_eps_merge_kernel(int64_t n_entries, const uint32_t *__restrict__ tab_df,
                                                             const unsigned long long *__restrict__ tab_first,
                                                             const BmEpsRound *__restrict__ r,
                                                             uint32_t *__restrict__ cursor, uint32_t *__restrict__ nt,
                                                             uint64_t *__restrict__ keys, uint64_t *__restrict__ vals,
                                                             int32_t *__restrict__ overflow) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_entries) return;
  const uint32_t df = tab_df[e];
  if (df == 0) return;
  const int j = (int)(e % kBmEpsFilters);
  int64_t cur = 0;
  int left = 0;
  const int64_t slot = bm25_eps_slot(r, j, 1, cursor, cur, left, overflow);
  if (slot < 0) return;
  keys[slot] = tab_first[e];
  vals[slot] = bm25_eps_val(j, df);
  atomicAdd(nt + j, 1u);
}

// Slot i of the round, sorted by `first`: its filter as a sort key (63: nobody filled the slot) and
// its idf.
__global__ void __launch_bounds__(256) bm25_eps_idf_kernel(int64_t n, const uint64_t *__restrict__ vals,
                                                           const BmEpsRound *__restrict__ r,
                                                           const double *__restrict__ logtab,
                                                           uint8_t *__restrict__ fkey, double *__restrict__ idf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = vals[i];
  const int j = (int)(v >> 56);
  uint8_t k = 63;
  double x = 0.0;
  if (j < r->n) {
    const int64_t df = (int64_t)(v & 0xffffffffull), nc = r->nc[j];
    if (df > 0 && df <= nc) {
      k = (uint8_t)j;
      x = logtab[nc - df] - logtab[df];
    }
  }
  fkey[i] = k;
  idf[i] = x;
}

// Workgroup j = one wave = filter j of the round: its nt[j] idfs follow those of the filters before
// it.  One accumulator, one chain of adds in the order of the array; every lane holds the same sum.
__global__ void __launch_bounds__(64) bm25_eps_sum_kernel(const double *__restrict__ idf, const uint32_t *__restrict__ nt,
                                                          const BmEpsRound *__restrict__ r,
                                                          BmEpsResult *__restrict__ res) {
  const int j = blockIdx.x, lane = threadIdx.x;
  int64_t at = 0;
  for (int i = 0; i < j; ++i) at += nt[i];
  const int64_t n = nt[j];
  double sum = 0.0;
  int64_t c = 0;
  for (; c + 64 <= n; c += 64) {
    const double v = idf[at + c + lane];
#pragma unroll
    for (int k = 0; k < 64; ++k) sum = sum + __shfl(v, k);
  }
  if (c < n) {
    const double v = c + lane < n ? idf[at + c + lane] : 0.0;
    for (int k = 0; k < (int)(n - c); ++k) sum = sum + __shfl(v, k);
  }
  if (lane == 0) res[r->out[j]] = BmEpsResult{sum, n};
}

// Rounds over filters 0 .. bound.size(): the first filter of every round, and the end.  Greedy, in
// order: a round takes filters while it holds fewer than kBmEpsFilters and their bounds, summed, stay
// within the budget; it always takes one.
inline std::vector<int32_t> bm25_eps_plan(const std::vector<int64_t> &bound, int64_t budget) {
  std::vector<int32_t> start;
  int64_t sum = 0;
  int32_t held = 0;
  for (size_t i = 0; i < bound.size(); ++i) {
    if (i == 0 || held == kBmEpsFilters || sum + bound[i] > budget) {
      start.push_back((int32_t)i);
      sum = 0;
      held = 0;
    }
    sum += bound[i];
    held += 1;
  }
  start.push_back((int32_t)bound.size());
  return start;
}

}  // namespace cm

namespace {

// eps[i] = the epsilon floor of the filter whose bitmap begins at allow_dev + allow_off[i], whose
// candidates number nc[i] and hold sum_len[i] tokens, for i < n.  Reads allow_dev, the index and the
// log table (grown here); writes h->eps_ws only.  h->last_eps_passes = the rounds it took.
int bm25_eps_multi(cm_bm25 *h, const uint32_t *allow_dev, int n, const int64_t *allow_off, const int64_t *nc,
                   const int64_t *sum_len, double *eps) {
  h->last_eps_passes = 0;
  std::vector<int32_t> who;   // filters with candidates: the others' epsilon is 0.0 (cm_bm25_filter_eps)
  std::vector<int64_t> bound;
  for (int i = 0; i < n; ++i) {
    eps[i] = 0.0;
    if (nc[i] <= 0) continue;
    who.push_back(i);
    // a term of the candidate vocabulary is one of the vocabulary's, owns a posting, and is a token of a candidate
    bound.push_back(std::min(std::min<int64_t>(sum_len[i], h->vocab), h->npost));
  }
  if (who.empty()) return CM_OK;
  if (h->npost <= 0) CM_FAIL(CM_EZERODIV, "float division by zero (candidate documents have no tokens)");
  int rc;
  if ((rc = bm25_grow_logtab(h, h->ndocs))) return rc;
  const std::vector<int32_t> start = bm25_eps_plan(bound, kBmEpsTupleBudget);
  const int n_rounds = (int)start.size() - 1;
  const int64_t ndocs = h->ndocs, n_slices = ceil_div(h->npost, kBmEpsSlice);
  int n_cu = 0;
  CM_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, h->dev));
  const int64_t post_blocks = std::min<int64_t>(ceil_div(n_slices, 4), 4 * (int64_t)std::max(n_cu, 1));
  const int64_t slack = post_blocks * 4 * kBmEpsChunk;   // slots a filter's cursor may hand out and leave unfilled
  const int doc_bits = 64 - __builtin_clzll((unsigned long long)ndocs);   // every row < ndocs fits
  // ---- the rounds, and the largest one's sizes ----
  std::vector<BmEpsRound> rounds((size_t)n_rounds);
  int64_t cap_max = 0;
  size_t sort_b = 16;
  for (int q = 0; q < n_rounds; ++q) {
    BmEpsRound &r = rounds[q];
    r = BmEpsRound{};
    r.n = start[q + 1] - start[q];
    for (int j = 0; j < r.n; ++j) {
      const int32_t i = who[start[q] + j];
      r.out[j] = start[q] + j;
      r.allow_off[j] = allow_off[i];
      r.nc[j] = nc[i];
      r.seg[j + 1] = r.seg[j] + bound[start[q] + j] + slack;
    }
    for (int j = r.n; j < kBmEpsFilters; ++j) r.seg[j + 1] = r.seg[j];
    const int64_t cap = r.seg[r.n];
    if (cap > INT32_MAX) CM_FAIL(CM_EUNSUPPORTED, "cm_bm25_filter_eps_multi: more than 2^31 tuple slots in one round");
    cap_max = std::max(cap_max, cap);
    size_t b1 = 0, b2 = 0;
    CM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                              (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)cap, 0, 32 + doc_bits,
                                              h->stream));
    CM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b2, (const uint8_t *)nullptr, (uint8_t *)nullptr,
                                              (const double *)nullptr, (double *)nullptr, (int)cap, 0, 6, h->stream));
    sort_b = std::max(sort_b, std::max(b1, b2));
  }
  // ---- workspace: a buffer of its own (ws, tmp and allow_buf hold a list search's live state) ----
  const int64_t n_entries = n_slices * kBmEpsFilters, n_who = (int64_t)who.size();
  BmEpsRound *rounds_dev;
  BmEpsResult *res_dev;
  int32_t *flag_dev;
  uint32_t *memb, *cursor, *nt, *tab_df;
  unsigned long long *tab_first;
  uint64_t *keys_a, *vals_a, *keys_b, *vals_b;
  uint8_t *fk_a, *fk_b;
  char *sort_ws;
  const auto carve = [&](char *base) {   // the bytes it takes
    Carver c{base};
    rounds_dev = c.take<BmEpsRound>((size_t)n_rounds);
    res_dev = c.take<BmEpsResult>((size_t)n_who);
    flag_dev = c.take<int32_t>(1);
    memb = c.take<uint32_t>((size_t)ndocs);
    // zeroed every round: the cursors, the tuple counts, the table's df (cursor up to tab_first)
    cursor = c.take<uint32_t>(kBmEpsFilters * kBmEpsCursorStride);
    nt = c.take<uint32_t>(kBmEpsFilters);
    tab_df = c.take<uint32_t>((size_t)n_entries);
    // set to ~0 every round: the table's first keys, the tuple slots (tab_first up to keys_b)
    tab_first = c.take<unsigned long long>((size_t)n_entries);
    keys_a = c.take<uint64_t>((size_t)cap_max);
    vals_a = c.take<uint64_t>((size_t)cap_max);
    keys_b = c.take<uint64_t>((size_t)cap_max);
    vals_b = c.take<uint64_t>((size_t)cap_max);
    fk_a = c.take<uint8_t>((size_t)cap_max);
    fk_b = c.take<uint8_t>((size_t)cap_max);
    sort_ws = c.take<char>(sort_b);
    return c.off;
  };
  if ((rc = h->eps_ws.ensure(carve(nullptr)))) return rc;
  carve(h->eps_ws.as<char>());
  double *idf_in = reinterpret_cast<double *>(keys_a), *idf_sorted = reinterpret_cast<double *>(vals_a);   // (free by then)
  CM_HIP(hipMemcpyAsync(rounds_dev, rounds.data(), rounds.size() * sizeof(BmEpsRound), hipMemcpyHostToDevice, h->stream));
  CM_HIP(hipMemsetAsync(flag_dev, 0, 4, h->stream));
  for (int q = 0; q < n_rounds; ++q) {
    const BmEpsRound *r = rounds_dev + q;
    const int64_t cap = rounds[q].seg[rounds[q].n];
    CM_HIP(hipMemsetAsync(cursor, 0, (char *)tab_first - (char *)cursor, h->stream));
    CM_HIP(hipMemsetAsync(tab_first, 0xff, (char *)keys_b - (char *)tab_first, h->stream));
    hipLaunchKernelGGL(bm25_eps_memb_kernel, dim3((unsigned)ceil_div(ndocs, 256)), dim3(256), 0, h->stream, allow_dev,
                       h->live.as<uint32_t>(), ndocs, r, memb);
    CM_HIP(hipGetLastError());
    hipLaunchKernelGGL(bm25_eps_post_kernel, dim3((unsigned)post_blocks), dim3(256), 0, h->stream,
                       h->term_off.as<int64_t>(), h->post_doc.as<int32_t>(), h->post_pos.as<uint32_t>(), h->vocab, h->npost,
                       n_slices, ndocs, memb, r, cursor, nt, tab_df, tab_first, keys_a, vals_a, flag_dev);
    CM_HIP(hipGetLastError());
    hipLaunchKernelGGL(bm25_eps_merge_kernel, dim3((unsigned)ceil_div(n_entries, 256)), dim3(256), 0, h->stream, n_entries,
                       tab_df, tab_first, r, cursor, nt, keys_a, vals_a, flag_dev);
    CM_HIP(hipGetLastError());
    size_t b = sort_b;
    CM_HIP(hipcub::DeviceRadixSort::SortPairs(sort_ws, b, keys_a, keys_b, vals_a, vals_b, (int)cap, 0, 32 + doc_bits,
                                              h->stream));
    hipLaunchKernelGGL(bm25_eps_idf_kernel, dim3((unsigned)ceil_div(cap, 256)), dim3(256), 0, h->stream, cap, vals_b, r,
                       h->logtab.as<double>(), fk_a, idf_in);
    CM_HIP(hipGetLastError());
    b = sort_b;
    CM_HIP(hipcub::DeviceRadixSort::SortPairs(sort_ws, b, fk_a, fk_b, idf_in, idf_sorted, (int)cap, 0, 6, h->stream));
    hipLaunchKernelGGL(bm25_eps_sum_kernel, dim3((unsigned)rounds[q].n), dim3(64), 0, h->stream, idf_sorted, nt, r, res_dev);
    CM_HIP(hipGetLastError());
  }
  // ---- the one read-back ----
  std::vector<BmEpsResult> res((size_t)n_who);
  int32_t flag = 0;
  CM_HIP(hipMemcpyAsync(res.data(), res_dev, res.size() * sizeof(BmEpsResult), hipMemcpyDeviceToHost, h->stream));
  CM_HIP(hipMemcpyAsync(&flag, flag_dev, 4, hipMemcpyDeviceToHost, h->stream));
  CM_HIP(hipStreamSynchronize(h->stream));
  h->last_eps_passes = n_rounds;
  if (flag) CM_FAIL(CM_EDEVICE, "cm_bm25_filter_eps_multi: a tuple segment overflowed its bound");
  for (int64_t u = 0; u < n_who; ++u) {
    if (res[u].count == 0) CM_FAIL(CM_EZERODIV, "float division by zero (candidate documents have no tokens)");
    eps[who[u]] = 0.25 * (res[u].sum / (double)res[u].count);
  }
  return CM_OK;
}

}  // namespace

extern "C" {

int cm_bm25_filter_eps_multi(cm_bm25 *h, const uint32_t *allow_bits, int32_t n_filters, double *eps_out) {
  if (!h || !allow_bits || !eps_out) CM_FAIL(CM_EINVAL, "NULL argument");
  if (n_filters < 0) CM_FAIL(CM_EINVAL, "cm_bm25_filter_eps_multi: n_filters must be >= 0");
  if (n_filters == 0) return CM_OK;
  const int64_t ndocs = h->ndocs, nw = ceil_div(ndocs, 32), total = (int64_t)n_filters * nw;
  if (total >= INT32_MAX)
    CM_FAIL(CM_EUNSUPPORTED, "cm_bm25_filter_eps_multi: n_filters x ceil(ndocs / 32) must stay below 2^31 - 1: split the batch");
  DeviceGuard dg(h->dev);
  h->last_eps_passes = 0;
  std::vector<int64_t> stat(2 * (size_t)n_filters, 0), allow_off((size_t)n_filters), nc((size_t)n_filters);
  std::vector<int64_t> sum_len((size_t)n_filters);
  int rc;
  if (total > 0) {
    if ((rc = h->allow_buf.ensure((size_t)total * 4)) || (rc = h->tmp.ensure(stat.size() * 8))) return rc;
    CM_HIP(hipMemcpyAsync(h->allow_buf.ptr, allow_bits, (size_t)total * 4, hipMemcpyDefault, h->stream));  // host or device
    CM_HIP(hipMemsetAsync(h->tmp.ptr, 0, stat.size() * 8, h->stream));
    for (int f = 0; f < n_filters; ++f) {   // {Nc, sum of lengths} of every filter, as cm_bm25_filter_eps takes its one
      hipLaunchKernelGGL(bm25_filtered_stats_kernel, dim3((unsigned)std::min<int64_t>(1024, ceil_div(nw, 256))), dim3(256),
                         0, h->stream, h->dl.as<int32_t>(), h->live.as<uint32_t>(), h->allow_buf.as<uint32_t>() + f * nw,
                         ndocs, h->tmp.as<unsigned long long>() + 2 * f);
      CM_HIP(hipGetLastError());
    }
    CM_HIP(hipMemcpyAsync(stat.data(), h->tmp.ptr, stat.size() * 8, hipMemcpyDeviceToHost, h->stream));
    CM_HIP(hipStreamSynchronize(h->stream));
  }
  for (int f = 0; f < n_filters; ++f) {
    allow_off[f] = f * nw;
    nc[f] = stat[2 * (size_t)f];
    sum_len[f] = stat[2 * (size_t)f + 1];
  }
  return bm25_eps_multi(h, h->allow_buf.as<uint32_t>(), n_filters, allow_off.data(), nc.data(), sum_len.data(), eps_out);
}

int32_t cm_bm25_last_eps_passes(cm_bm25 *h) { return h ? h->last_eps_passes : -1; }

}  // extern "C"
