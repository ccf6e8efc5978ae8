// Row-list search (cm_dense_search_lists; included by cm_dense.hip): a batch whose queries carry
// different where clauses (ChromaVectorStore.query, rag/retrieval/vector_chroma.py:204-253, called
// once per question by the reference).  The scans take one bitmap per launch and stream the whole
// store for it; a clause that allows a few thousand rows is answered here without a scan:
//   1. lists  the allowed live rows of every filter as ascending CSR lists (cm_row_lists.h).  The
//             list lengths are read back once (the function's one synchronisation before its
//             outputs): they size the key buffers.
//   2. scan   dense_list_scan_kernel: one workgroup per (filter, kListChunk rows of its list, tile of
//             up to kListQT of the queries that use it).  The query tile sits in LDS; every wave
//             gathers whole fp32 rows, kListRowsPerWave at a time, float4 per lane across the dims,
//             and computes dense_all_keys_kernel's distance in fp64.  Key (f32_order(dist) << 32 | row)
//             of list element e of query i goes to keys[seg_off[i] + e].
//   3. top-k  one segmented radix sort (hipCUB) over the queries' segments, then the first k keys of
//             every segment: ascending (distance, row), pads (0.f, -1) past the segment's end, the
//             finish of dense_search_full.
// No scan, seed, re-rank or plane is touched; only C and the live bitmap are read.
// cm_dense_search_lists_dev is the same body with the queries and the results on the device: the
// padded queries and their fp64 norms come from list_query_prep_kernel instead of the host loop, the
// top-k kernel writes the caller's tensors, and the handle's stream first waits for the caller's.

namespace cm {

constexpr int kListChunk = 256;       // rows of one list per workgroup (tests restate it)
constexpr int kListQT = 8;            // queries per tile at most: 32 fp64 accumulators per lane (the fold needs 4 x 8)
constexpr int kListRowsPerWave = 4;   // rows in flight per wave
constexpr int kListLdsBytes = 49152;  // query tile budget: three workgroups per CU

// queries per tile at this ld: the tile (qt x ld fp32) stays within kListLdsBytes
__host__ __device__ inline int list_query_tile(int ld) {
  const int fit = kListLdsBytes / (ld * 4);
  return fit < 1 ? 1 : fit > kListQT ? kListQT : fit;
}

// One work item of the list scan: list `filter`, its rows [chunk * kListChunk, ...), and the nqt
// queries qorder[q0 .. q0 + nqt).
struct ListItem {
  int32_t filter, chunk, q0, nqt;
};

// The hot kernel.  256 threads = 4 waves; the query tile (nqt x ld fp32) in LDS.  A wave takes
// kListRowsPerWave list rows at a time: all their float4 loads of a dim step are issued before the
// first use (the gather shape of compact_gather_kernel), each row is read once from HBM for the whole
// tile.  fp64 dot products and row norms with dense_all_keys_kernel's lane mapping and butterfly, so
// a row's distance to a query is the value cm_dense_search's k > cm_max_topk path computes.
__global__ void __launch_bounds__(256) dense_list_scan_kernel(
    const float *__restrict__ C, int ld, const uint32_t *__restrict__ rows, const int64_t *__restrict__ list_off,
    const ListItem *__restrict__ items, const int32_t *__restrict__ qorder, const int32_t *__restrict__ seg_off,
    const float *__restrict__ qp, const double *__restrict__ qnorm, uint64_t *__restrict__ keys) {
  extern __shared__ float4 s_q[];   // [nqt][ld / 4]
  const ListItem it = items[blockIdx.x];
  const int nqt = it.nqt;
  const int ld4 = ld >> 2;
  for (int i = threadIdx.x; i < nqt * ld4; i += 256) {
    const int j = i / ld4;
    s_q[i] = reinterpret_cast<const float4 *>(qp + (int64_t)qorder[it.q0 + j] * ld)[i - j * ld4];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t lo = list_off[it.filter];
  const int64_t len = list_off[it.filter + 1] - lo;
  const int64_t e0 = (int64_t)it.chunk * kListChunk;
  const int64_t e1 = min(e0 + (int64_t)kListChunk, len);
  for (int64_t e = e0 + (threadIdx.x >> 6) * kListRowsPerWave; e < e1; e += 4 * kListRowsPerWave) {
    const int nr = (int)min((int64_t)kListRowsPerWave, e1 - e);   // wave-uniform
    const float *cr[kListRowsPerWave];
    uint32_t r[kListRowsPerWave];
#pragma unroll
    for (int u = 0; u < kListRowsPerWave; ++u) {
      r[u] = rows[lo + e + min(u, nr - 1)];
      cr[u] = C + (int64_t)r[u] * ld;
    }
    double dq[kListRowsPerWave * kListQT], dc[kListRowsPerWave];   // dq[u * kListQT + j]
#pragma unroll
    for (int u = 0; u < kListRowsPerWave; ++u) {
      dc[u] = 0.0;
#pragma unroll
      for (int j = 0; j < kListQT; ++j) dq[u * kListQT + j] = 0.0;
    }
    for (int c = lane; c < ld4; c += 64) {
      float4 x[kListRowsPerWave];
#pragma unroll
      for (int u = 0; u < kListRowsPerWave; ++u) x[u] = reinterpret_cast<const float4 *>(cr[u])[c];
#pragma unroll
      for (int u = 0; u < kListRowsPerWave; ++u)
        dc[u] += (double)x[u].x * x[u].x + (double)x[u].y * x[u].y + (double)x[u].z * x[u].z +
                 (double)x[u].w * x[u].w;
#pragma unroll
      for (int j = 0; j < kListQT; ++j) {
        if (j < nqt) {   // block-uniform
          const float4 y = s_q[j * ld4 + c];
#pragma unroll
          for (int u = 0; u < kListRowsPerWave; ++u)
            dq[u * kListQT + j] += (double)x[u].x * y.x + (double)x[u].y * y.y + (double)x[u].z * y.z + (double)x[u].w * y.w;
        }
      }
    }
    // Cross-lane sums.  32 butterflies of six steps each would cost more than the dot products, so
    // the sums are folded as they are reduced: at offset o a lane keeps the half of the accumulators
    // its bit o selects and hands the other half to lane ^ o.  Each kept value is own + partner's,
    // the butterfly's operands exactly, so the bits are the butterfly's.  After offsets 32..2 a lane
    // holds one accumulator, pair (u, j) = lane >> 1, summed over the 32 lanes that agree with it in
    // bit 0; offset 1 completes it.  The four row norms fold the same way over offsets 32 and 16 and
    // land on their own u (= lane >> 4), then take the plain butterfly.
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int half = 16 >> s, o = 32 >> s;
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int i = 0; i < half; ++i) {
        const double keep = up ? dq[i + half] : dq[i];
        const double send = up ? dq[i] : dq[i + half];
        dq[i] = keep + __shfl_xor(send, o);
      }
      if (s < 2) {
        const int h2 = 2 >> s;
#pragma unroll
        for (int i = 0; i < h2; ++i) {
          const double keep = up ? dc[i + h2] : dc[i];
          const double send = up ? dc[i] : dc[i + h2];
          dc[i] = keep + __shfl_xor(send, o);
        }
      } else {
        dc[0] += __shfl_xor(dc[0], o);
      }
    }
    const double my_dq = dq[0] + __shfl_xor(dq[0], 1);
    const double my_dc = dc[0] + __shfl_xor(dc[0], 1);
    const int u = lane >> 4, j = (lane >> 1) & (kListQT - 1);
    if (!(lane & 1) && u < nr && j < nqt) {
      const int qi = qorder[it.q0 + j];
      const float dist = (float)(1.0 - my_dq / ((sqrt(my_dc) + 1e-30) * (qnorm[qi] + 1e-30)));
      uint32_t row = r[0];
#pragma unroll
      for (int v = 1; v < kListRowsPerWave; ++v) row = u == v ? r[v] : row;
      keys[(int64_t)seg_off[qi] + e + u] = ((uint64_t)f32_order(dist) << 32) | (uint64_t)row;
    }
  }
}

// out[i][j] = the j-th key of query i's sorted segment; (0.f, -1) past its end.
__global__ void __launch_bounds__(256) list_topk_kernel(const uint64_t *__restrict__ sorted,
                                                        const int32_t *__restrict__ seg_off, int nq, int k,
                                                        float *__restrict__ out_dist, int64_t *__restrict__ out_row) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)nq * k) return;
  const int i = (int)(idx / k), j = (int)(idx - (int64_t)i * k);
  const int32_t s0 = seg_off[i];
  if (j < seg_off[i + 1] - s0) {
    const uint64_t key = sorted[(int64_t)s0 + j];
    out_dist[idx] = f32_unorder((uint32_t)(key >> 32));
    out_row[idx] = (int64_t)(uint32_t)key;
  } else {
    out_dist[idx] = 0.f;
    out_row[idx] = -1;
  }
}

// Padded queries and their fp64 norms from device queries (cm_dense_search_lists_dev): one workgroup
// per query.  qp[i][0 .. ld) = q[i][0 .. dim) then zeros; qnorm[i] = sqrt of the host loop's sum --
// s += (double)v * v over the dims in order, ONE sequential chain (a tree gives other bits), the
// products exact in fp64.  The block stages kListNormChunk dims at a time in LDS with coalesced
// loads, thread 0 adds them in order.
constexpr int kListNormChunk = 2048;

__global__ void __launch_bounds__(256) list_query_prep_kernel(const float *__restrict__ q, int dim, int ld,
                                                              float *__restrict__ qp, double *__restrict__ qnorm) {
  __shared__ float s_v[kListNormChunk];
  const float *src = q + (int64_t)blockIdx.x * dim;
  float *dst = qp + (int64_t)blockIdx.x * ld;
  double s = 0.0;
  for (int c0 = 0; c0 < ld; c0 += kListNormChunk) {
    const int n = min(kListNormChunk, ld - c0);
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += 256) {
      const float v = c0 + c < dim ? src[c0 + c] : 0.f;
      s_v[c] = v;
      dst[c0 + c] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = min(n, dim - c0);   // the pads add nothing: left out, as on the host
      for (int c = 0; c < m; ++c) {
        const double v = (double)s_v[c];
        s += v * v;
      }
    }
  }
  if (threadIdx.x == 0) qnorm[blockIdx.x] = __dsqrt_rn(s);
}

// cm_dense_search_lists and cm_dense_search_lists_dev: one body.  on_dev: q, out_dist and out_row
// are device memory, and `stream` (the caller's) is waited for before the handle's stream starts.
static int dense_search_lists_impl(const char *fn, bool on_dev, cm_dense *h, const float *q, int32_t nq, int32_t k,
                                   const uint32_t *allow_bits, int32_t n_filters, const int32_t *filter_of,
                                   float *out_dist, int64_t *out_row, float *out_vec, hipStream_t stream) {
  const std::string F(fn);
  // ---- argument checks: host only, before any device call ----
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (nq < 1) CM_FAIL(CM_EINVAL, F + ": nq must be >= 1");
  if (k < 1) CM_FAIL(CM_EINVAL, F + ": k must be >= 1");
  if (n_filters < 1) CM_FAIL(CM_EINVAL, F + ": n_filters must be >= 1");
  if (!q || !allow_bits || !filter_of || !out_dist || !out_row) CM_FAIL(CM_EINVAL, "NULL argument");
  int rc;
  if ((rc = check_filter_of(F, filter_of, nq, n_filters))) return rc;
  if (k > kMaxTopK)
    CM_FAIL(CM_EUNSUPPORTED, F + ": k above cm_max_topk(): use cm_dense_search per clause");
  DeviceGuard dg(h->dev);
  const int64_t size = h->size;
  const int ld = h->ld, dim = h->dim;
  if (on_dev && (rc = stream_wait_stream(h->stream, stream))) return rc;   // the producers of q and allow_bits
  // ---- 1. list lengths: count, scan, read back ----
  RowLists lists;
  if ((rc = row_lists_count(F, "size", allow_bits, n_filters, h->live, nullptr, size, h->allow_buf, h->rows_buf, h->stream,
                            lists)))
    return rc;
  const int64_t *off = lists.stat.data();
  // ---- the queries' segments and the work items (host) ----
  const int64_t n_rows = off[n_filters];
  std::vector<int32_t> seg, qorder((size_t)nq), qstart((size_t)n_filters + 1, 0);
  int64_t n_keys = 0;
  if ((rc = row_list_segments(F, off, filter_of, nq, seg, n_keys))) return rc;
  for (int i = 0; i < nq; ++i) qstart[filter_of[i] + 1] += 1;
  for (int f = 0; f < n_filters; ++f) qstart[f + 1] += qstart[f];
  {
    std::vector<int32_t> fill(qstart.begin(), qstart.end() - 1);
    for (int i = 0; i < nq; ++i) qorder[fill[filter_of[i]]++] = i;   // grouped by filter, ascending inside
  }
  const int qt = list_query_tile(ld);
  std::vector<ListItem> items;
  for (int f = 0; f < n_filters; ++f) {
    const int64_t len = off[f + 1] - off[f];
    const int nqf = qstart[f + 1] - qstart[f];
    if (len == 0 || nqf == 0) continue;
    for (int64_t c = 0; c < ceil_div(len, kListChunk); ++c)
      for (int t = 0; t < nqf; t += qt)   // the tiles of one chunk are neighbours: its rows come from L2
        items.push_back(ListItem{f, (int32_t)c, qstart[f] + t, std::min(qt, nqf - t)});
  }
  if (items.size() > (size_t)INT32_MAX)
    CM_FAIL(CM_EUNSUPPORTED, F + ": too many work items: split the batch");
  // ---- workspace ----
  size_t sort_b = 0;
  if (n_keys > 0)
    CM_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_b, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                      (int)n_keys, nq, (const int32_t *)nullptr,
                                                      (const int32_t *)nullptr, 0, 64, h->stream));
  char *sort_ws;
  uint32_t *rows;
  ListItem *items_dev;
  int32_t *qord_dev, *seg_dev;
  float *qp;
  double *qn_dev;
  uint64_t *keys, *sorted;
  const auto carve = [&](char *base) {   // the bytes it takes; called to size ws first: ensure may move it
    Carver c{base};
    sort_ws = c.take<char>(sort_b);
    rows = c.take<uint32_t>((size_t)n_rows);
    items_dev = c.take<ListItem>(items.size());
    qord_dev = c.take<int32_t>((size_t)nq);
    seg_dev = c.take<int32_t>((size_t)nq + 1);
    qp = c.take<float>((size_t)nq * ld);
    qn_dev = c.take<double>((size_t)nq);
    keys = c.take<uint64_t>((size_t)n_keys);
    sorted = c.take<uint64_t>((size_t)n_keys);
    return c.off;
  };
  const size_t obytes = (size_t)nq * k * (4 + 8);
  const size_t vbytes = out_vec ? (size_t)nq * k * dim * 4 : 0;
  if ((rc = h->ws.ensure(carve(nullptr)))) return rc;
  if (!on_dev && (rc = h->out_buf.ensure(round_up(obytes, 256) + vbytes))) return rc;
  carve(h->ws.as<char>());
  // (device form: the top-k kernel writes the caller's tensors)
  float *d_dist = on_dev ? out_dist : h->out_buf.as<float>();
  int64_t *d_row = on_dev ? out_row : reinterpret_cast<int64_t *>(h->out_buf.as<char>() + round_up((int64_t)nq * k * 4, 8));
  CM_HIP(hipMemcpyAsync(seg_dev, seg.data(), seg.size() * 4, hipMemcpyHostToDevice, h->stream));
  std::vector<float> qpad;   // host sources of the copies below: alive until the last synchronise
  std::vector<double> qn;
  if (n_keys > 0) {
    // queries padded to ld, and their norms in fp64: dense_search_full's
    if (on_dev) {
      hipLaunchKernelGGL(list_query_prep_kernel, dim3((unsigned)nq), dim3(256), 0, h->stream, q, dim, ld, qp, qn_dev);
      CM_HIP(hipGetLastError());
    } else {
      qpad.assign((size_t)nq * ld, 0.f);
      qn.resize((size_t)nq);
      for (int i = 0; i < nq; ++i) {
        double s = 0.0;
        for (int c = 0; c < dim; ++c) {
          const float v = q[(int64_t)i * dim + c];
          qpad[(size_t)i * ld + c] = v;
          s += (double)v * v;
        }
        qn[i] = std::sqrt(s);
      }
      CM_HIP(hipMemcpyAsync(qp, qpad.data(), qpad.size() * 4, hipMemcpyHostToDevice, h->stream));
      CM_HIP(hipMemcpyAsync(qn_dev, qn.data(), qn.size() * 8, hipMemcpyHostToDevice, h->stream));
    }
    CM_HIP(hipMemcpyAsync(qord_dev, qorder.data(), qorder.size() * 4, hipMemcpyHostToDevice, h->stream));
    CM_HIP(hipMemcpyAsync(items_dev, items.data(), items.size() * 16, hipMemcpyHostToDevice, h->stream));
    // ---- 1b. the lists ----
    if ((rc = row_lists_scatter(lists, h->live, size, rows, h->stream))) return rc;
    // ---- 2. exact keys ----
    h->timer.begin(h->stream);
    hipLaunchKernelGGL(dense_list_scan_kernel, dim3((unsigned)items.size()), dim3(256), (size_t)qt * ld * 4, h->stream,
                       h->C, ld, rows, lists.off_dev, items_dev, qord_dev, seg_dev, qp, qn_dev, keys);
    CM_HIP(hipGetLastError());
    h->timer.end(h->stream);
    // ---- 3. top-k ----
    CM_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(sort_ws, sort_b, keys, sorted, (int)n_keys, nq, seg_dev,
                                                      seg_dev + 1, 0, 64, h->stream));
  }
  hipLaunchKernelGGL(list_topk_kernel, dim3((unsigned)ceil_div((int64_t)nq * k, 256)), dim3(256), 0, h->stream,
                     sorted, seg_dev, nq, k, d_dist, d_row);
  CM_HIP(hipGetLastError());
  float *d_vec = nullptr;
  if (out_vec) {
    d_vec = reinterpret_cast<float *>(h->out_buf.as<char>() + round_up(obytes, 256));
    if ((rc = cm_dense_gather_dev(h, d_row, (int64_t)nq * k, d_vec, h->stream))) return rc;
  }
  if (!on_dev) {
    CM_HIP(hipMemcpyAsync(out_dist, d_dist, (size_t)nq * k * 4, hipMemcpyDeviceToHost, h->stream));
    CM_HIP(hipMemcpyAsync(out_row, d_row, (size_t)nq * k * 8, hipMemcpyDeviceToHost, h->stream));
    if (out_vec) CM_HIP(hipMemcpyAsync(out_vec, d_vec, vbytes, hipMemcpyDeviceToHost, h->stream));
  }
  CM_HIP(hipStreamSynchronize(h->stream));   // the host sources above, and the outputs: complete on return
  return CM_OK;
}

}  // namespace cm

extern "C" {

int cm_dense_search_lists(cm_dense *h, const float *q, int32_t nq, int32_t k, const uint32_t *allow_bits,
                          int32_t n_filters, const int32_t *filter_of, float *out_dist, int64_t *out_row,
                          float *out_vec) {
  return dense_search_lists_impl("cm_dense_search_lists", false, h, q, nq, k, allow_bits, n_filters, filter_of, out_dist,
                                 out_row, out_vec, nullptr);
}

int cm_dense_search_lists_dev(cm_dense *h, const float *q_dev, int32_t nq, int32_t k, const uint32_t *allow_bits,
                              int32_t n_filters, const int32_t *filter_of, float *dist_dev, int64_t *row_dev,
                              void *stream) {
  return dense_search_lists_impl("cm_dense_search_lists_dev", true, h, q_dev, nq, k, allow_bits, n_filters, filter_of,
                                 dist_dev, row_dev, nullptr, static_cast<hipStream_t>(stream));
}

}  // extern "C"
