// cm_bm25_remove / cm_bm25_remove_dev: documents removed without a rebuild (included by cm_bm25.hip).
//
// Removing documents drops their postings and moves every later row down by the number of removed
// rows before it.  The move is monotone, so each term's surviving postings keep their order and the
// CSR is a stream compaction of the old one:
//   ranks   keep words (~remove, masked to ndocs), their popcounts, a library exclusive scan:
//           new_row(d) = rank_w[d >> 5] + popc(keep[d >> 5] & lowmask(d & 31)).  Two arrays of
//           ndocs / 8 bytes; no N-sized map.
//   pass A  one wave per 64 consecutive postings ballots "this posting's document is kept" into
//           smask[] (u64) and its popcount into sbase[], which a library exclusive scan (in place)
//           turns into each group's first output posting; the last entry is the surviving total.
//   offsets term_off'[t] = sbase[p >> 6] + popc(smask[p >> 6] & lowmask(p & 63)), p = term_off[t]:
//           O(1) per term, whatever its posting count.
//   pass B  the same division by postings: a surviving lane writes its renumbered document, tf and
//           position at sbase + popc(lower survivors); a wave's survivors are consecutive.
// Two passes with a scan between them, not one pass with a look-back between workgroups: no
// workgroup ever waits for another, stream order is the only synchronisation.  The price is a
// second read of post_doc.  Pass A, the offsets and the steps around them are the plan all three
// mutations share: cm_bm25_mutate.inc.
//
// Peak device memory: old + new postings (10 B each) plus 16 B per 64 postings (smask, sbase); the
// old arrays are freed when the call returns.

namespace cm {

// One thread per 32 rows: keep word and its popcount (cnt[], scanned into the rank words by the
// caller); tot[0] += removed rows that were live, tot[1] += their lengths (sum_len counts live
// documents only; a dead row of a tombstoned build has a length but no postings).
__global__ void __launch_bounds__(256) bm25_rm_keep_kernel(const uint32_t *__restrict__ remove,
                                                           const uint32_t *__restrict__ live,
                                                           const int32_t *__restrict__ dl, int64_t ndocs, int64_t nw,
                                                           uint32_t *__restrict__ keep, int32_t *__restrict__ cnt,
                                                           unsigned long long *__restrict__ tot) {
  __shared__ unsigned long long s_live[256 / 64], s_len[256 / 64];
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long n_gone = 0, len_gone = 0;
  if (w < nw) {
    const int64_t left = ndocs - w * 32;
    const uint32_t valid = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
    const uint32_t rm = remove[w] & valid;
    keep[w] = ~rm & valid;
    cnt[w] = __popc(~rm & valid);
    uint32_t gone = rm & live[w];
    n_gone = (unsigned long long)__popc(gone);
    while (gone) {
      const int b = __ffs((int)gone) - 1;
      gone &= gone - 1;
      len_gone += (unsigned long long)dl[w * 32 + b];
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_gone += __shfl_down(n_gone, o);
    len_gone += __shfl_down(len_gone, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_live[threadIdx.x >> 6] = n_gone;
    s_len[threadIdx.x >> 6] = len_gone;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 256 / 64; ++i) {
      n_gone += s_live[i];
      len_gone += s_len[i];
    }
    if (n_gone) atomicAdd(&tot[0], n_gone);
    if (len_gone) atomicAdd(&tot[1], len_gone);
  }
}

// Pass B: the survivors of group g go to out[sbase[g] ...), in order, with their new row numbers.
__global__ void __launch_bounds__(kRmThreads) bm25_rm_compact_kernel(
    const int32_t *__restrict__ post_doc, const uint16_t *__restrict__ post_tf, const uint32_t *__restrict__ post_pos,
    int64_t npost, const uint32_t *__restrict__ keep, const int32_t *__restrict__ rank_w,
    const unsigned long long *__restrict__ smask, const int64_t *__restrict__ sbase, int32_t *__restrict__ out_doc,
    uint16_t *__restrict__ out_tf, uint32_t *__restrict__ out_pos) {
  const int lane = threadIdx.x & 63;
  const int64_t g0 = ((int64_t)blockIdx.x * (kRmThreads / 64) + (threadIdx.x >> 6)) * kRmGroups;
#pragma unroll
  for (int u = 0; u < kRmGroups; ++u) {
    const int64_t g = g0 + u, p = g * 64 + lane;
    if (g * 64 >= npost) break;
    const unsigned long long m = smask[g];  // (bits of postings at or beyond npost are clear)
    if ((m >> lane) & 1ull) {
      const int64_t q = sbase[g] + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
      const int32_t d = post_doc[p];
      out_doc[q] = rank_w[d >> 5] + __popc(keep[d >> 5] & ((1u << (d & 31)) - 1u));
      out_tf[q] = post_tf[p];
      out_pos[q] = post_pos[p];
    }
  }
}

// dl' and live': one thread per 32 old rows.  Its kept rows are consecutive new rows from
// rank_w[w] on, so their live bits fall into at most two words of out_live (zeroed by the caller).
__global__ void bm25_rm_rows_kernel(const uint32_t *__restrict__ keep, const int32_t *__restrict__ rank_w,
                                    const uint32_t *__restrict__ live, const int32_t *__restrict__ dl, int64_t nw,
                                    int32_t *__restrict__ out_dl, uint32_t *__restrict__ out_live) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  uint32_t k = keep[w];
  if (!k) return;
  const uint32_t lv = live[w];
  const int32_t r = rank_w[w];
  unsigned long long acc = 0;
  int i = 0;
  while (k) {
    const int b = __ffs((int)k) - 1;
    k &= k - 1;
    out_dl[r + i] = dl[w * 32 + b];
    acc |= (unsigned long long)((lv >> b) & 1u) << i;
    ++i;
  }
  acc <<= (r & 31);  // (i <= 32 bits, shifted by < 32)
  if ((uint32_t)acc) atomicOr(&out_live[r >> 5], (uint32_t)acc);
  if (acc >> 32) atomicOr(&out_live[(r >> 5) + 1], (uint32_t)(acc >> 32));
}

}  // namespace cm

namespace {

// The shared device path: h->ndocs > 0 rows, remove_bits_dev (ceil(ndocs / 32) words) readable on
// `st`.
int bm25_remove_device(cm_bm25 *h, const uint32_t *remove_bits_dev, hipStream_t st) {
  const int64_t n0 = h->ndocs, p0 = h->npost, nw = ceil_div(n0, 32);
  const int32_t vocab = h->vocab;
  int rc;
  CM_HIP(hipStreamSynchronize(h->stream));  // earlier work on the handle's stream read the old arrays
  // -- row ranks
  TmpBuf keep, cnt, rank_w, tot, cub_tmp;
  if ((rc = keep.ensure((size_t)nw * 4)) || (rc = cnt.ensure(((size_t)nw + 1) * 4)) ||
      (rc = rank_w.ensure(((size_t)nw + 1) * 4)) || (rc = tot.ensure(16)))
    return rc;
  CM_HIP(hipMemsetAsync(tot.ptr, 0, 16, st));
  CM_HIP(hipMemsetAsync(cnt.as<int32_t>() + nw, 0, 4, st));
  hipLaunchKernelGGL(bm25_rm_keep_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, st, remove_bits_dev,
                     h->live.as<uint32_t>(), h->dl.as<int32_t>(), n0, nw, keep.as<uint32_t>(), cnt.as<int32_t>(),
                     tot.as<unsigned long long>());
  CM_HIP(hipGetLastError());
  if ((rc = bm25_exclusive_sum(cub_tmp, cnt.as<int32_t>(), rank_w.as<int32_t>(), nw + 1, st))) return rc;
  int32_t n1_32 = 0;
  int64_t gone[2] = {0, 0};  // removed rows that were live, their lengths
  CM_HIP(hipMemcpyAsync(&n1_32, rank_w.as<int32_t>() + nw, 4, hipMemcpyDeviceToHost, st));
  CM_HIP(hipMemcpyAsync(gone, tot.ptr, 16, hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  const int64_t n1 = n1_32;
  if (n1 == n0) return CM_OK;  // no bit set below ndocs
  if (n1 == 0) return cm_bm25_build(h, nullptr, nullptr, 0, vocab, nullptr);  // every document: the build of none
  // -- pass A and the scan: which postings survive, and where each group of 64 goes (cm_bm25_timing:
  // pass A with its scan, then pass B, one pair each)
  Survivors s;
  if ((rc = bm25_survivor_pass(h, keep.as<uint32_t>(), cub_tmp, s, st))) return rc;
  const int64_t p1 = s.n;
  FreshArrays f;
  if ((rc = bm25_fresh_alloc(f, vocab, p1, n1)) || (rc = bm25_fresh_offsets(h, f, vocab, &s, nullptr, st))) return rc;
  if (p0 > 0) {
    h->timer.begin(st);
    hipLaunchKernelGGL(bm25_rm_compact_kernel, dim3((unsigned)ceil_div(p0, kRmChunk)), dim3(kRmThreads), 0, st,
                       h->post_doc.as<int32_t>(), h->post_tf.as<uint16_t>(), h->post_pos.as<uint32_t>(), p0,
                       keep.as<uint32_t>(), rank_w.as<int32_t>(), s.mask(), s.base(), f.doc.as<int32_t>(),
                       f.tf.as<uint16_t>(), f.pos.as<uint32_t>());
    h->timer.end(st);
    CM_HIP(hipGetLastError());
  }
  CM_HIP(hipMemsetAsync(f.live.ptr, 0, (size_t)ceil_div(n1, 32) * 4, st));
  hipLaunchKernelGGL(bm25_rm_rows_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, st, keep.as<uint32_t>(),
                     rank_w.as<int32_t>(), h->live.as<uint32_t>(), h->dl.as<int32_t>(), nw, f.dl.as<int32_t>(),
                     f.live.as<uint32_t>());
  CM_HIP(hipGetLastError());
  return bm25_install(h, f, n1, p1, vocab, -gone[0], -gone[1], st);
}

}  // namespace

extern "C" {

int cm_bm25_remove_dev(cm_bm25 *h, const uint32_t *remove_bits_dev, void *stream) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (h->ndocs == 0) return CM_OK;
  if (!remove_bits_dev) CM_FAIL(CM_EINVAL, "remove_bits_dev is NULL");
  DeviceGuard dg(h->dev);
  return bm25_remove_device(h, remove_bits_dev, (hipStream_t)stream);
}

int cm_bm25_remove(cm_bm25 *h, const int64_t *rows, int64_t n_rows) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (n_rows < 0) CM_FAIL(CM_EINVAL, "n_rows must be >= 0");
  if (n_rows == 0) return CM_OK;
  if (!rows) CM_FAIL(CM_EINVAL, "rows is NULL");
  std::vector<uint32_t> bits;
  int rc = bm25_rows_to_bits(rows, n_rows, h->ndocs, false, bits);
  if (rc) return rc;
  DeviceGuard dg(h->dev);
  // only the bitmap goes up; the rest is the device path
  TmpBuf up;
  if ((rc = up.ensure(bits.size() * 4))) return rc;
  CM_HIP(hipMemcpyAsync(up.ptr, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, h->stream));
  return bm25_remove_device(h, up.as<uint32_t>(), h->stream);
}

}  // extern "C"
