// Compaction of the dense store (cm_dense_compact / cm_dense_truncate; included by cm_dense.hip).
// The reference's vacuum_indexes (rag/admin/backup.py:178-202) calls vec_store.compact() when the
// vector store has one; col.delete (rag/retrieval/vector_chroma.py:181-187) only clears a live bit
// here, so without this a deleted row keeps its HBM (fp32 row, both coarse planes, scales) and is
// streamed by every later scan.
//
// cm_dense_compact moves the live rows of [0, size) to [0, n) in ascending order, in place:
//   1. rank   popcount per live word, exclusive scan (hipCUB), old_of_new[rank(r)] = r for every
//             live row r: the gather list and the map handed back to the caller.
//   2. move   C and invc, chunk by chunk, through a device staging buffer: the source rows of new
//             rows [d0, d0 + m) are gathered into staging, then staging is copied to [d0, d0 + m).
//             Both steps run on h->stream: stream order is the only synchronisation.
//             Why in place is safe.  old_of_new is strictly increasing, so old_of_new[i] >= i: every
//             row moves down or stays.  A chunk's destination [d0, d0 + m) therefore holds only
//             (a) old rows that earlier chunks already moved away (or dead rows), and (b) source
//             rows of this same chunk -- and those are all in staging before the first write,
//             because the copy is enqueued after the gather.  Source rows of later chunks are new
//             rows >= d0 + m, so their old index is >= d0 + m as well: no chunk overwrites a row
//             that a later chunk still has to read.  Rows before the first dead row satisfy
//             old_of_new[i] == i and are skipped.
//   3. planes Xh, Xq and rmeta are not moved: the 16-row scale groups and 64-row tiles change
//             membership, so they are recomputed from the moved fp32 rows with the upsert's kernels
//             (dense_replane_kernel, dense_q8_group_kernel: bit-identical to a fresh upsert of the
//             same rows), from the 64-row tile of the first dead row on.  rnorm holds running
//             maxima over every row ever written; it is left as it is: a maximum that is too large
//             only widens the certificate's band (more re-ranked rows, never a wrong result).
//   4. tail   cm_dense_truncate's body: live bits = ones for [0, n), zero above; everything at rows
//             >= n cleared as in a never-written store.
//   5. shrink (optional) the arrays are reallocated at round_up(max(n, kStepRows), kStepRows) rows
//             through dense_realloc, the code dense_grow uses.

namespace cm {

// cnt[w] = live rows of word w among rows < size; cnt[n_words] = 0 (so the exclusive scan's last
// element is the total).
__global__ void __launch_bounds__(256) compact_count_kernel(const uint32_t *__restrict__ live, int64_t size,
                                                            int64_t n_words, int64_t *__restrict__ cnt) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w > n_words) return;
  uint32_t bits = 0;
  if (w < n_words) {
    bits = live[w];
    const int64_t left = size - w * 32;
    if (left < 32) bits &= (1u << left) - 1u;
  }
  cnt[w] = __popc(bits);
}

// old_of_new[prefix[w] + j] = row of the j-th live bit of word w; first_dead = the lowest dead row
// (stays `size` when there is none).
__global__ void __launch_bounds__(256) compact_rank_kernel(const uint32_t *__restrict__ live, int64_t size,
                                                           int64_t n_words, const int64_t *__restrict__ prefix,
                                                           int64_t *__restrict__ old_of_new,
                                                           unsigned long long *__restrict__ first_dead) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_words) return;
  const int64_t left = size - w * 32;
  const uint32_t valid = left < 32 ? (1u << left) - 1u : 0xffffffffu;
  uint32_t bits = live[w] & valid;
  const uint32_t dead = ~bits & valid;
  if (dead) atomicMin(first_dead, (unsigned long long)(w * 32 + __ffs(dead) - 1));
  int64_t o = prefix[w];
  while (bits) {
    const int b = __ffs(bits) - 1;
    old_of_new[o++] = w * 32 + b;
    bits &= bits - 1;
  }
}

// Gather m rows of C (and their invc) into staging: out row i = C row src[i].  Pure bandwidth: one
// wave per 4 rows, the lanes across a row's float4s (1 KiB contiguous per wave-instruction, a 768-d
// row = 3 of them), the loads of all 4 rows issued before the first store; grid-stride over the
// row quads.  ld is a multiple of 128, so ld / 4 is a multiple of 32 and every access is 16-byte
// aligned.  No LDS.
constexpr int kCompactRowsPerWave = 4;
__global__ void __launch_bounds__(256) compact_gather_kernel(const float *__restrict__ C,
                                                             const float *__restrict__ invc, int ld,
                                                             const int64_t *__restrict__ src, int64_t m,
                                                             float *__restrict__ outC, float *__restrict__ outI) {
  const int lane = threadIdx.x & 63;
  const int ld4 = ld >> 2;
  const int64_t n_quads = ceil_div(m, kCompactRowsPerWave);
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  for (int64_t qd = wave0; qd < n_quads; qd += n_waves) {
    const int64_t i0 = qd * kCompactRowsPerWave;
    const int nr = (int)min((int64_t)kCompactRowsPerWave, m - i0);   // wave-uniform
    int64_t r[kCompactRowsPerWave];
#pragma unroll
    for (int u = 0; u < kCompactRowsPerWave; ++u) r[u] = src[i0 + min(u, nr - 1)];
    for (int c = lane; c < ld4; c += 64) {
      f32x4 v[kCompactRowsPerWave];
#pragma unroll
      for (int u = 0; u < kCompactRowsPerWave; ++u) v[u] = reinterpret_cast<const f32x4 *>(C + r[u] * ld)[c];
#pragma unroll
      for (int u = 0; u < kCompactRowsPerWave; ++u)
        if (u < nr) reinterpret_cast<f32x4 *>(outC + (i0 + u) * ld)[c] = v[u];
    }
    if (lane < nr) outI[i0 + lane] = invc[src[i0 + lane]];
  }
}

// Live words [w0, w1): ones for rows < n, zero above.  keep != 0 (truncate): a row that was dead
// below n stays dead (AND); keep == 0 (compact): rows [0, n) are all live.
__global__ void __launch_bounds__(256) compact_live_kernel(uint32_t *__restrict__ live, int64_t w0, int64_t w1,
                                                           int64_t n, int keep) {
  const int64_t w = w0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= w1) return;
  const int64_t left = n - w * 32;
  const uint32_t mask = left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << left) - 1u;
  live[w] = keep ? (live[w] & mask) : mask;
}

// Column sums of xn = c * invc (the planes' fp32 normalisation) over the live rows of [0, size), in
// fp64: the mean a caller hands to cm_dense_set_center.  One workgroup per fixed range of
// kMeanRowsPerWg rows, wave w its rows 4 i + w, the lanes across a row's float4s (16-byte loads, as
// compact_gather_kernel), four rows' loads in flight per wave; a dead row is skipped by its live
// word, which is wave-uniform (one row per wave at a time).  The waves' sums meet in LDS in wave
// order and go to part[wg][ld]; dense_mean_reduce_kernel adds the workgroups' partials in index
// order.  No floating-point atomics and a geometry that depends on size alone: two calls on the
// same store return the same bits.  One pass over the fp32 rows, HBM-bound.
constexpr int kMeanRowsPerWg = 2048;
constexpr int kMeanSlots = 8;   // float4 slots per lane: ld <= 2048
__global__ void __launch_bounds__(256) dense_mean_kernel(const float *__restrict__ C, const float *__restrict__ invc,
                                                         const uint32_t *__restrict__ live, int64_t size, int ld,
                                                         double *__restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ld4 = ld >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * kMeanRowsPerWg;
  const int64_t r1 = min(r0 + kMeanRowsPerWg, size);
  double acc[kMeanSlots][4];
#pragma unroll
  for (int s = 0; s < kMeanSlots; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[s][e] = 0.0;
  constexpr int U = 4;   // rows in flight per wave
  for (int64_t rb = r0 + wave; rb < r1; rb += 4 * U) {
    int64_t r[U];
    bool on[U];
    float inv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      r[u] = rb + 4 * u;
      on[u] = r[u] < r1 && ((live[r[u] >> 5] >> (r[u] & 31)) & 1u);   // wave-uniform
      inv[u] = on[u] ? invc[r[u]] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < kMeanSlots; ++s) {
      const int c = lane + 64 * s;
      if (c < ld4) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          v[u] = on[u] ? reinterpret_cast<const f32x4 *>(C + r[u] * ld)[c] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (on[u]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[s][e] += (double)(v[u][e] * inv[u]);
          }
      }
    }
  }
  __shared__ double s_sum[3][2048];   // waves 1-3; wave 0 adds them in order
  if (wave > 0) {
#pragma unroll
    for (int s = 0; s < kMeanSlots; ++s)
      if (lane + 64 * s < ld4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s_sum[wave - 1][4 * (lane + 64 * s) + e] = acc[s][e];
      }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int s = 0; s < kMeanSlots; ++s)
      if (lane + 64 * s < ld4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = 4 * (lane + 64 * s) + e;
          part[(int64_t)blockIdx.x * ld + col] = ((acc[s][e] + s_sum[0][col]) + s_sum[1][col]) + s_sum[2][col];
        }
      }
  }
}
__global__ void __launch_bounds__(256) dense_mean_reduce_kernel(const double *__restrict__ part, int n_wg, int ld,
                                                                double *__restrict__ sums) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= ld) return;
  double t = 0.0;
  for (int w = 0; w < n_wg; ++w) t += part[(int64_t)w * ld + col];
  sums[col] = t;
}

}  // namespace cm

namespace {

// frees its device memory at scope exit (the compaction's scratch is not kept on the handle)
struct ScopedDevBuf : DevBuf {
  ~ScopedDevBuf() { release(); }
};

// Rows per chunk of the move: kBounceBytes of staging by default; CM_COMPACT_CHUNK_ROWS (read at
// every call, for tests) = any positive row count.
int64_t compact_chunk_rows(const cm_dense *h) {
  if (const char *e = getenv("CM_COMPACT_CHUNK_ROWS")) {
    const long long v = atoll(e);
    if (v > 0) return (int64_t)v;
  }
  return std::max<int64_t>(1, (int64_t)kBounceBytes / ((int64_t)h->ld * 4 + 4));
}

// The body of cm_dense_truncate on h->stream (no synchronisation): rows >= n of [0, extent) cleared
// as in a never-written store, size = n.  fill_live: live bits of [0, n) all set (compaction) instead
// of kept.  The planes are tile-major, so whole 64-row tiles at and above round_up(n, 64) are
// zeroed with memsets; the tile that n cuts keeps rows below n: its rows >= n get a zero f16 image
// (dense_replane_kernel over the zeroed fp32 rows), and its four scale groups, which interleave
// within the tile (q8_group_row), are re-quantised, since the rows they lost may have set their scale.
int dense_truncate_stream(cm_dense *h, int64_t n, bool fill_live) {
  const int64_t extent = std::min<int64_t>(round_up(h->size, kStepRows), h->rows_alloc);  // rows ever written
  const int64_t ld = h->ld;
  if (n < extent) {
    CM_HIP(hipMemsetAsync(h->C + n * ld, 0, (size_t)(extent - n) * ld * 4, h->stream));
    CM_HIP(hipMemsetAsync(h->invc + n, 0, (size_t)(extent - n) * 4, h->stream));
  }
  const int64_t w0 = fill_live ? 0 : n >> 5, w1 = extent / 32;
  if (w1 > w0)
    hipLaunchKernelGGL(compact_live_kernel, dim3((unsigned)ceil_div(w1 - w0, 256)), dim3(256), 0, h->stream, h->live,
                       w0, w1, n, fill_live ? 0 : 1);
  CM_HIP(hipGetLastError());
  const int64_t t1 = std::min<int64_t>(round_up(n, 64), extent);   // first whole tile above n
  if (n < t1) {
    const int64_t hi = std::min<int64_t>(t1, h->xh_rows);
    if (n < hi)
      hipLaunchKernelGGL(dense_replane_kernel, dim3((unsigned)(hi - n)), dim3(256), 0, h->stream, h->C, h->invc, n,
                         hi - n, h->dim, h->ld, h->Xh);
    CM_HIP(hipGetLastError());
    hipLaunchKernelGGL(dense_q8_group_kernel, dim3(4), dim3(256), 0, h->stream, h->C, h->invc,
                       dense_mu(h), (const uint32_t *)h->live, (const int64_t *)nullptr, (n >> 6) * 4, (int64_t)4, h->dim, h->ld, h->Xq, h->rmeta,
                       reinterpret_cast<uint32_t *>(h->rnorm));
    CM_HIP(hipGetLastError());
  }
  if (t1 < extent) {
    const int64_t xh_hi = std::min<int64_t>(extent, h->xh_rows);
    if (t1 < xh_hi) CM_HIP(hipMemsetAsync(h->Xh + t1 * ld, 0, (size_t)(xh_hi - t1) * ld * 2, h->stream));
    CM_HIP(hipMemsetAsync(h->Xq + t1 * ld, 0, (size_t)(extent - t1) * ld, h->stream));
    CM_HIP(hipMemsetAsync(h->rmeta + t1, 0, (size_t)(extent - t1) * 8, h->stream));
  }
  h->size = n;
  return CM_OK;
}

// shrink: reallocate at the rows the store needs when that is smaller; device to device when old
// and new fit with kGrowSlack to spare, else through the host.  A store that fits neither way
// keeps its arrays: not an error.
int dense_shrink(cm_dense *h) {
  const int64_t cap = round_up(std::max<int64_t>(h->size, kStepRows), kStepRows);
  if (cap >= h->rows_alloc) return CM_OK;
  size_t free_b = 0, total_b = 0;
  const bool fits = hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                    (int64_t)free_b >= dense_row_bytes(h, cap) + kGrowSlack;
  const int64_t size = h->size;
  const int rc = dense_realloc(h, cap, !fits && size > 0);
  if (rc == CM_ENOMEM && h->C && h->size == size) return CM_OK;   // the rows are still there
  return rc;
}

}  // namespace

extern "C" {

int cm_dense_truncate(cm_dense *h, int64_t new_size) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (new_size < 0 || new_size > h->size) CM_FAIL(CM_EINVAL, "cm_dense_truncate: new_size must be in [0, size]");
  if (new_size == h->size) return CM_OK;
  DeviceGuard dg(h->dev);
  CM_HIP(hipDeviceSynchronize());   // searches and device upserts run on the callers' streams
  const int rc = dense_truncate_stream(h, new_size, false);
  if (rc) return rc;
  CM_HIP(hipStreamSynchronize(h->stream));
  return CM_OK;
}

int cm_dense_compact(cm_dense *h, int64_t expect_live, int32_t shrink, int64_t *old_rows_out, int64_t *new_size) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  DeviceGuard dg(h->dev);
  CM_HIP(hipDeviceSynchronize());   // searches and device upserts run on the callers' streams
  const int64_t size = h->size;
  const int64_t nw = ceil_div(size, 32);
  int64_t n = 0;
  unsigned long long first_dead = (unsigned long long)size;
  int rc;
  ScopedDevBuf rank_buf, scan_tmp, stage;
  int64_t *old_of_new = nullptr;
  if (size > 0) {
    // ---- 1. rank (reads only) ----
    const size_t cnt_b = (size_t)round_up((nw + 1) * 8, 256);
    const size_t map_b = (size_t)round_up(size * 8, 256);
    if ((rc = rank_buf.ensure(2 * cnt_b + map_b + 256))) return rc;
    int64_t *cnt = rank_buf.as<int64_t>();
    int64_t *prefix = reinterpret_cast<int64_t *>(rank_buf.as<char>() + cnt_b);
    old_of_new = reinterpret_cast<int64_t *>(rank_buf.as<char>() + 2 * cnt_b);
    unsigned long long *fd_dev = reinterpret_cast<unsigned long long *>(rank_buf.as<char>() + 2 * cnt_b + map_b);
    size_t tmp_b = 0;
    CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_b, cnt, prefix, (int)(nw + 1), h->stream));
    if ((rc = scan_tmp.ensure(std::max<size_t>(tmp_b, 16)))) return rc;
    h->timer.begin(h->stream);
    CM_HIP(hipMemcpyAsync(fd_dev, &first_dead, 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)ceil_div(nw + 1, 256)), dim3(256), 0, h->stream, h->live,
                       size, nw, cnt);
    CM_HIP(hipGetLastError());
    CM_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp.ptr, tmp_b, cnt, prefix, (int)(nw + 1), h->stream));
    hipLaunchKernelGGL(compact_rank_kernel, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0, h->stream, h->live, size,
                       nw, prefix, old_of_new, fd_dev);
    CM_HIP(hipGetLastError());
    h->timer.end(h->stream);
    CM_HIP(hipMemcpyAsync(&n, prefix + nw, 8, hipMemcpyDeviceToHost, h->stream));
    CM_HIP(hipMemcpyAsync(&first_dead, fd_dev, 8, hipMemcpyDeviceToHost, h->stream));
    CM_HIP(hipStreamSynchronize(h->stream));
  }
  if (expect_live >= 0 && expect_live != n)
    CM_FAIL(CM_EINVAL, "cm_dense_compact: the store holds " + std::to_string(n) + " live rows, the caller expected " +
                           std::to_string(expect_live));
  const int64_t f = std::min<int64_t>((int64_t)first_dead, n);   // rows [0, f) are in place
  const int64_t chunk = std::max<int64_t>(1, std::min(compact_chunk_rows(h), n - f));
  if (f < n && (rc = stage.ensure((size_t)chunk * ((size_t)h->ld * 4 + 4)))) return rc;
  // ---- nothing was modified up to here ----
  if (old_rows_out && n > 0) {
    CM_HIP(hipMemcpyAsync(old_rows_out, old_of_new, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    CM_HIP(hipStreamSynchronize(h->stream));
  }
  if (n < size) {
    // ---- 2. move (the in-place argument: top of this file) ----
    h->timer.begin(h->stream);
    float *stC = stage.as<float>();
    float *stI = stC + (size_t)chunk * h->ld;
    for (int64_t d0 = f; d0 < n; d0 += chunk) {
      const int64_t m = std::min(chunk, n - d0);
      const int64_t blocks = std::min<int64_t>(ceil_div(m, 4 * kCompactRowsPerWave), 4 * (int64_t)num_cus(h->dev));
      hipLaunchKernelGGL(compact_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->C, h->invc, h->ld,
                         old_of_new + d0, m, stC, stI);
      CM_HIP(hipGetLastError());
      CM_HIP(hipMemcpyAsync(h->C + d0 * h->ld, stC, (size_t)m * h->ld * 4, hipMemcpyDeviceToDevice, h->stream));
      CM_HIP(hipMemcpyAsync(h->invc + d0, stI, (size_t)m * 4, hipMemcpyDeviceToDevice, h->stream));
    }
    h->timer.end(h->stream);
    // ---- 3. planes of the moved rows: whole tiles here, the tile that n cuts in the tail step ----
    h->timer.begin(h->stream);
    const int64_t t0 = (f >> 6) << 6;
    const int64_t xh_hi = std::min<int64_t>(n, h->xh_rows);
    if (t0 < xh_hi)
      hipLaunchKernelGGL(dense_replane_kernel, dim3((unsigned)(xh_hi - t0)), dim3(256), 0, h->stream, h->C, h->invc, t0,
                         xh_hi - t0, h->dim, h->ld, h->Xh);
    CM_HIP(hipGetLastError());
    const int64_t g_lo = (t0 >> 6) * 4, g_hi = (n >> 6) * 4;
    if (g_lo < g_hi)
      hipLaunchKernelGGL(dense_q8_group_kernel, dim3((unsigned)(g_hi - g_lo)), dim3(256), 0, h->stream, h->C, h->invc,
                         dense_mu(h), (const uint32_t *)nullptr, (const int64_t *)nullptr, g_lo, g_hi - g_lo, h->dim, h->ld, h->Xq, h->rmeta,
                         reinterpret_cast<uint32_t *>(h->rnorm));
    CM_HIP(hipGetLastError());
    // ---- 4. live bits and the tail ----
    if ((rc = dense_truncate_stream(h, n, true))) return rc;
    h->timer.end(h->stream);
    CM_HIP(hipStreamSynchronize(h->stream));
  }
  if (new_size) *new_size = n;
  if (shrink) return dense_shrink(h);
  return CM_OK;
}

// The int8 plane's centre (cm_dense_q8.inc, "Centred plane").  Every group that was ever written is
// re-quantised in this call, which is what makes zeroing rnorm[2] (otherwise never lowered) safe: the
// groups above hold only code 0 and add nothing to it.
int cm_dense_set_center(cm_dense *h, const float *mu) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (mu) {
    double n2 = 0.0;
    for (int c = 0; c < h->dim; ++c) {
      if (!std::isfinite(mu[c])) CM_FAIL(CM_EINVAL, "cm_dense_set_center: non-finite entry");
      n2 += (double)mu[c] * (double)mu[c];
    }
    if (!(n2 <= 1.0)) CM_FAIL(CM_EINVAL, "cm_dense_set_center: ||mu|| must be <= 1");
  }
  DeviceGuard dg(h->dev);
  CM_HIP(hipDeviceSynchronize());   // searches and device upserts run on the callers' streams
  std::vector<float> pad((size_t)h->ld, 0.f);
  if (mu) std::copy(mu, mu + h->dim, pad.begin());
  CM_HIP(hipMemcpyAsync(h->mu_dev, pad.data(), (size_t)h->ld * 4, hipMemcpyHostToDevice, h->stream));
  h->centred = mu != nullptr;
  if (mu) h->mu.assign(mu, mu + h->dim);
  else h->mu.clear();
  const int64_t extent = std::min<int64_t>(round_up(h->size, kStepRows), h->rows_alloc);  // rows ever written
  if (extent > 0) {
    CM_HIP(hipMemsetAsync(h->rnorm + 2, 0, 4, h->stream));
    hipLaunchKernelGGL(dense_q8_group_kernel, dim3((unsigned)(extent / 16)), dim3(256), 0, h->stream, h->C, h->invc,
                       dense_mu(h), (const uint32_t *)h->live, (const int64_t *)nullptr, (int64_t)0, extent / 16, h->dim, h->ld, h->Xq, h->rmeta,
                       reinterpret_cast<uint32_t *>(h->rnorm));
    CM_HIP(hipGetLastError());
  }
  CM_HIP(hipStreamSynchronize(h->stream));   // (pad is read by the copy until here)
  return CM_OK;
}

int cm_dense_get_center(cm_dense *h, float *mu_out, int32_t *is_set) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (is_set) *is_set = h->centred ? 1 : 0;
  if (mu_out)
    for (int c = 0; c < h->dim; ++c) mu_out[c] = h->centred ? h->mu[(size_t)c] : 0.f;
  return CM_OK;
}

int cm_dense_column_sums(cm_dense *h, double *sums_out, int64_t *n_live_out) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (!sums_out) CM_FAIL(CM_EINVAL, "cm_dense_column_sums: sums_out is NULL");
  DeviceGuard dg(h->dev);
  CM_HIP(hipDeviceSynchronize());   // device upserts run on the callers' streams
  const int64_t n_live = cm_dense_live_count(h);
  if (n_live < 0) CM_FAIL(CM_EDEVICE, "cm_dense_column_sums: live count failed");
  if (n_live_out) *n_live_out = n_live;
  std::fill(sums_out, sums_out + h->dim, 0.0);
  if (n_live == 0) return CM_OK;
  const int n_wg = (int)ceil_div(h->size, kMeanRowsPerWg);
  ScopedDevBuf part;
  int rc;
  if ((rc = part.ensure(((size_t)n_wg + 1) * h->ld * 8))) return rc;
  double *pd = part.as<double>(), *sums = pd + (size_t)n_wg * h->ld;
  h->timer.begin(h->stream);
  hipLaunchKernelGGL(dense_mean_kernel, dim3((unsigned)n_wg), dim3(256), 0, h->stream, h->C, h->invc, h->live, h->size,
                     h->ld, pd);
  CM_HIP(hipGetLastError());
  hipLaunchKernelGGL(dense_mean_reduce_kernel, dim3((unsigned)ceil_div(h->ld, 256)), dim3(256), 0, h->stream, pd, n_wg,
                     h->ld, sums);
  CM_HIP(hipGetLastError());
  h->timer.end(h->stream);
  CM_HIP(hipMemcpyAsync(sums_out, sums, (size_t)h->dim * 8, hipMemcpyDeviceToHost, h->stream));
  CM_HIP(hipStreamSynchronize(h->stream));
  return CM_OK;
}

int cm_dense_mean(cm_dense *h, float *mean_out, int64_t *n_live_out) {
  if (!h) CM_FAIL(CM_EINVAL, "null handle");
  if (!mean_out) CM_FAIL(CM_EINVAL, "cm_dense_mean: mean_out is NULL");
  std::vector<double> sums((size_t)h->dim);
  int64_t n = 0;
  const int rc = cm_dense_column_sums(h, sums.data(), &n);
  if (rc) return rc;
  for (int c = 0; c < h->dim; ++c) mean_out[c] = n > 0 ? (float)(sums[(size_t)c] / (double)n) : 0.f;
  if (n_live_out) *n_live_out = n;
  return CM_OK;
}

}  // extern "C"
