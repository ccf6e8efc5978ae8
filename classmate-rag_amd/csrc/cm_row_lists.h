// Step 1 of the row-list searches (cm_dense_lists.inc, cm_bm25_lists.inc): the allowed live rows of
// every where clause of a batch as ascending CSR lists, built on the device.  A count per (filter,
// word) of allow[f][w] & live[w], one exclusive scan (hipCUB) over all the counts, one read-back of
// the lists' offsets (they size the caller's key buffers), then a scatter of the row numbers.
// cm_dense.hip and cm_bm25.hip both include this file into one shared object: everything in it has
// internal linkage.
#pragma once
#include "cm_common.h"

#include <hipcub/hipcub.hpp>

namespace cm {
namespace {

__device__ inline uint32_t row_list_word(const uint32_t *__restrict__ allow, const uint32_t *__restrict__ live,
                                         int64_t size, int64_t n_words, int64_t f, int64_t w) {
  uint32_t bits = allow[f * n_words + w] & live[w];
  const int64_t left = size - w * 32;
  if (left < 32) bits &= (1u << left) - 1u;
  return bits;
}

// Workgroup b = (filter b / nbw, words [256 (b % nbw), ...)): cnt[f * n_words + w] = rows of word w
// that filter f allows and that are live, among rows < size; cnt[n_filters * n_words] = 0 (the
// exclusive scan's last element = all list entries).  kSumLen: sum_len[f] += their lengths (zeroed
// by the caller).
template <bool kSumLen>
__global__ void __launch_bounds__(256) row_list_count_kernel(const uint32_t *__restrict__ allow,
                                                             const uint32_t *__restrict__ live,
                                                             const int32_t *__restrict__ dl, int64_t size,
                                                             int64_t n_words, int64_t nbw, int64_t total,
                                                             int64_t *__restrict__ cnt,
                                                             unsigned long long *__restrict__ sum_len) {
  const int64_t f = blockIdx.x / nbw, w = (blockIdx.x % nbw) * 256 + threadIdx.x;
  uint32_t bits = w < n_words ? row_list_word(allow, live, size, n_words, f, w) : 0u;
  if (w < n_words) cnt[f * n_words + w] = __popc(bits);
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[total] = 0;
  if constexpr (kSumLen) {
    __shared__ unsigned long long red[4];
    unsigned long long sum = 0;
    while (bits) {
      sum += (unsigned long long)dl[w * 32 + (__ffs(bits) - 1)];
      bits &= bits - 1;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long s = red[0] + red[1] + red[2] + red[3];
      if (s) atomicAdd(sum_len + f, s);
    }
  }
}

// off[f] = prefix[f * n_words] for f <= n_filters: where each list starts (CSR), contiguous (and
// followed by the length sums) for the one read-back.
__global__ void __launch_bounds__(256) row_list_offsets_kernel(const int64_t *__restrict__ prefix, int64_t n_words,
                                                               int n_filters, int64_t *__restrict__ off) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f <= n_filters) off[f] = prefix[(int64_t)f * n_words];
}

// rows[prefix[i] + j] = row of the j-th set bit of (filter, word) i: every list ascending.  Row:
// uint32_t or int32_t, the same bits (rows are below 2^31).
template <typename Row>
__global__ void __launch_bounds__(256) row_list_scatter_kernel(const uint32_t *__restrict__ allow,
                                                               const uint32_t *__restrict__ live, int64_t size,
                                                               int64_t n_words, int64_t total,
                                                               const int64_t *__restrict__ prefix,
                                                               Row *__restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t w = i % n_words;
  uint32_t bits = row_list_word(allow, live, size, n_words, i / n_words, w);
  int64_t o = prefix[i];
  while (bits) {
    rows[o++] = (Row)(w * 32 + (__ffs(bits) - 1));
    bits &= bits - 1;
  }
}

// What row_lists_count leaves behind.  The device pointers stay null when the store is empty.
struct RowLists {
  int64_t n_words = 0, total = 0;                  // words per bitmap; n_filters x n_words
  const uint32_t *allow = nullptr;                 // device: the bitmaps, rows of n_words words
  int64_t *prefix = nullptr, *off_dev = nullptr;   // device: the scan; off[0 .. n_filters] then the length sums
  std::vector<int64_t> stat;   // host: off[0 .. n_filters], then sum_len[0 .. n_filters) (zeros without dl)
};

// Count, scan, offsets and the one read-back, on `st`; returns after synchronising it.  allow_bits
// (host or device, n_filters rows of ceil(size / 32) words) is copied into allow_buf; the counts,
// the scan, the offsets and hipCUB's scratch live in `scratch`.  dl (nullable): the rows' lengths,
// summed per list.  size_name: what `size` is called in the caller's message.
inline int row_lists_count(const std::string &F, const char *size_name, const uint32_t *allow_bits, int n_filters,
                           const uint32_t *live, const int32_t *dl, int64_t size, DevBuf &allow_buf, DevBuf &scratch,
                           hipStream_t st, RowLists &L) {
  const int64_t nw = ceil_div(size, 32), total = (int64_t)n_filters * nw;
  if (total + 1 > INT32_MAX)
    CM_FAIL(CM_EUNSUPPORTED, F + ": n_filters x ceil(" + size_name + " / 32) must stay below 2^31: split the batch");
  L.n_words = nw;
  L.total = total;
  L.stat.assign(2 * (size_t)n_filters + 1, 0);
  if (total == 0) return CM_OK;
  size_t scan_b = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (const int64_t *)nullptr, (int64_t *)nullptr,
                                          (int)(total + 1), st));
  int64_t *cnt = nullptr;
  char *scan = nullptr;
  const auto carve = [&](char *base) {   // the bytes it takes
    Carver c{base};
    cnt = c.take<int64_t>((size_t)total + 1);
    L.prefix = c.take<int64_t>((size_t)total + 1);
    L.off_dev = c.take<int64_t>(L.stat.size());
    scan = c.take<char>(scan_b);
    return c.off;
  };
  int rc;
  if ((rc = allow_buf.ensure((size_t)total * 4)) || (rc = scratch.ensure(carve(nullptr)))) return rc;
  carve(scratch.as<char>());
  L.allow = allow_buf.as<uint32_t>();
  unsigned long long *sum_dev = reinterpret_cast<unsigned long long *>(L.off_dev + n_filters + 1);
  CM_HIP(hipMemcpyAsync(allow_buf.ptr, allow_bits, (size_t)total * 4, hipMemcpyDefault, st));  // host or device
  if (dl) CM_HIP(hipMemsetAsync(sum_dev, 0, (size_t)n_filters * 8, st));
  const int64_t nbw = ceil_div(nw, 256);
  hipLaunchKernelGGL(dl ? row_list_count_kernel<true> : row_list_count_kernel<false>, dim3((unsigned)(nbw * n_filters)),
                     dim3(256), 0, st, L.allow, live, dl, size, nw, nbw, total, cnt, sum_dev);
  CM_HIP(hipGetLastError());
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(scan, scan_b, cnt, L.prefix, (int)(total + 1), st));
  hipLaunchKernelGGL(row_list_offsets_kernel, dim3((unsigned)ceil_div(n_filters + 1, 256)), dim3(256), 0, st, L.prefix, nw,
                     n_filters, L.off_dev);
  CM_HIP(hipGetLastError());
  CM_HIP(hipMemcpyAsync(L.stat.data(), L.off_dev, (dl ? L.stat.size() : (size_t)n_filters + 1) * 8, hipMemcpyDeviceToHost,
                        st));
  CM_HIP(hipStreamSynchronize(st));
  return CM_OK;
}

// rows[off[f] ..) = list f, ascending, for every filter; only where a list holds a row (total > 0).
template <typename Row>
inline int row_lists_scatter(const RowLists &L, const uint32_t *live, int64_t size, Row *rows, hipStream_t st) {
  hipLaunchKernelGGL(row_list_scatter_kernel<Row>, dim3((unsigned)ceil_div(L.total, 256)), dim3(256), 0, st, L.allow, live,
                     size, L.n_words, L.total, L.prefix, rows);
  CM_HIP(hipGetLastError());
  return CM_OK;
}

// filter_of[i] in [0, n_filters) for every query (host; no device call).
inline int check_filter_of(const std::string &F, const int32_t *filter_of, int nq, int n_filters) {
  for (int i = 0; i < nq; ++i)
    if (filter_of[i] < 0 || filter_of[i] >= n_filters)
      CM_FAIL(CM_EINVAL, F + ": filter_of[" + std::to_string(i) + "] = " + std::to_string(filter_of[i]) +
                             " is outside [0, n_filters)");
  return CM_OK;
}

// The queries' key segments: seg[i + 1] - seg[i] = the length of query i's list; n_keys = seg[nq].
inline int row_list_segments(const std::string &F, const int64_t *off, const int32_t *filter_of, int nq,
                             std::vector<int32_t> &seg, int64_t &n_keys) {
  seg.assign((size_t)nq + 1, 0);
  n_keys = 0;
  for (int i = 0; i < nq; ++i) {
    n_keys += off[filter_of[i] + 1] - off[filter_of[i]];
    if (n_keys > INT32_MAX) CM_FAIL(CM_EUNSUPPORTED, F + ": more than 2^31 (query, row) pairs: split the batch");
    seg[i + 1] = (int32_t)n_keys;
  }
  return CM_OK;
}

}  // namespace
}  // namespace cm
