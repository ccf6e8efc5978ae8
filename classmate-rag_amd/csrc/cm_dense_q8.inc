// K1q: coarse int8 scan + per-row certified re-rank -- included by cm_dense.hip inside namespace
// cm, after K1c / K1s (VERDICT r3 #6: one byte per element instead of K1c's two).
//
// Plane Xq.  Every row's normalised vector xn = c * invc (hnswlib normalize_vector, as K1c's Xh)
// is quantised with its own scale
//     s_r = max|xn| / 127,   q8 = rint(xn / s_r) in [-127, 127],
// and stored fragment-major for v_mfma_i32_16x16x64_i8: 64-row tiles x 128-k chunks (8 KiB, the
// unit of one LDS-DMA ring slot), block b = 2 rt + kh (1 KiB) = rows 16 rt .. + 15 x k 64 kh .. + 63
// of the chunk; lane (g, j) of a block holds row 16 rt + j, its 16 bytes the k of q8_k6(g, e).
// Per row rmeta = {s_r, e_r}, e_r >= ||xn - s_r q8|| (fp64, rounded up); rnorm[2] = the largest
// ||s_r q8|| of any row (never lowered).  The query side is quantised the same way (dense_prep_q8).
//
// Bound.  The scan's coarse distance is d~ = 1 - s_q s_r acc, acc = sum q8_r q8_q (exact int32).
// xn.qn - x~.q~ = (xn - x~).qn + x~.(qn - q~), so for every row and query
//     |(1 - xn.qn) - d~| <= E_r = ||qn|| e_r + max||x~|| e_q + slack,
// the slack (4e-6) covering the fp32 rounding of d~, of qn / xn against the fp64 normalisation
// of the exact re-rank, and of E_r itself.  The bound is per ROW: at 10M x 768 the certified band
// was ~800 rows per query for the bench's E5 queries with per-row scales (a global max||e_r|| gives
// ~4,000; tools/int8_band.py, profiles/r04_int8_band_rowE.json); with the group scales below it is
// 1,190 rows from kth_up alone and 200 with the re-rank's pilot bound (profiles/rerank_pilot.txt).
//
//
// The slack by row stride n = ld (768; 1024 for dims 897-1024; 384 for dims 257-384), u = 2^-24.  What
// depends on n, as 768 (1024; 384):
//   the norms.  invc and the query's inv come from an fp32 sum of squares -- per thread a chain of
//     ceil(n / 256) terms (3, 4, 2), then 6 shuffle steps and 2 adds -- so the sum carries
//     <= (ceil(n / 256) + 8) u relative, its square root half of that, and sqrtf, the + 1e-30 and the
//     reciprocal <= u each: the common factor of xn (qn) against the fp64 normalisation is off by
//     <= ((ceil(n / 256) + 8) / 2 + 3) u = 8.5 u (9 u; 8 u), and each component's product rounding adds
//     u by Cauchy-Schwarz.  Both operands: |xn.qn - x^.q^| <= 19 u = 1.13e-6 (20 u = 1.19e-6; 18 u =
//     1.07e-6);
//   acc.  |acc| <= 127^2 n = 12 387 072 (16 516 096; 6 193 536) < 2^24, so (float)acc is exact at every
//     stride (it stops being so at n = 1152: a stride above 1024 needs a split or an int bound instead);
//   the fp64 sums of e_r, e_q, ||qn||, m_q and of the re-rank carry n 2^-53 <= 1.2e-13 relative
//     (4.3e-14 at 384), far inside the (1 + 1e-6) factors they are rounded up by.
//   What does not: A = fl32(s_q S) (u on |A acc| <= 1.02), the fma of lo (u: |lo| < 2), the two
//     roundings of B (u together, B < 1), a_q + b_q e_r (under u), the returned float (u, see
//     kQPilotPad): <= 4.1 u = 2.5e-7; W's own 1e-6 covers lo + W and the factor 2.
//   Sum: 1.38e-6 at 768, 1.44e-6 at 1024 -- one u more for the longer chains --, 1.32e-6 at 384 -- one
//   u less for the shorter ones -- against 4e-6.  The centre's terms (below) do not depend on n except
//   m_q's fp64 sum, smaller at 384.  The constants (4e-6, the centre's 5e-7, W's 1e-6) are therefore
//   the same at every stride, and every 768 and 1024 value keeps its bits.
//
// Centred plane (cm_dense_set_center).  Embedding models such as E5 put every vector near one
// dominant direction (pairwise cosine 0.7-0.9): the distances around the k-th best then spread
// several times less than on isotropic rows while e_r stays what it was, and the band grows until
// the (range, query) buffers overflow.  With a centre mu (dim floats, ||mu|| <= 1, usually the mean
// of the normalised rows) the plane stores q8(y), y = fl32(xn - mu), and rmeta, the group scale and
// rnorm[2] are those of y; dense_prep_q8 adds the constant back per query: m_q = mu.qn (fp64, from
// the fp32 qn), base_q = fl32(1 - m_q), and the scans' coarse distance is d~ = base_q - s_q s_r acc.
// xn.qn = y.qn + mu.qn + (xn - mu - y).qn, so the bound keeps its form with e_r, max||x~|| of y:
// both shrink with ||xn - mu|| ~ sqrt(1 - cos), and m_q is one constant per query, so the order of
// the coarse distances is that of y.qn.  The seed, every key and the re-rank stay in true-distance
// space and read uncentred data (f16 plane, fp32 rows).
// A row whose fp32 data is all zero (never written, truncated, or a stored zero vector) has xn = 0,
// true distance 1: it gets code 0 (d~ = base_q, off by |m_q| <= ||mu|| ||qn||) and e_r = ||mu||, and
// stays out of its group's scale, which |mu| would otherwise set for every partly filled group
// (a dead zero row, a hole, gets e_r = 0: dense_q8_group_kernel).
// Slack with a centre, added to a_q on top of the 4e-6 (5e-7, dense_prep_q8):
//   y = fl32(xn - mu), one rounding per component (__fsub_rn, never contracted with xn = c invc):
//     |y_c - (xn_c - mu_c)| <= 2^-24 |xn_c - mu_c|, on the dot product <= 2^-24 ||xn - mu|| ||qn||
//     <= 2^-24 * 2 * (1 + 1e-6)                                                   < 1.2e-7;
//   m_q: the term qn-against-the-fp64-normalisation is the plain plane's xn.(q^ - qn), already in the
//     4e-6 (xn.q^ = xn.(q^ - qn) + y.qn + mu.qn + ...: mu multiplies the same fp32 qn the codes were
//     made from), so only the fp64 sum's own rounding is new: <= ld * 2^-53 * ||mu|| ||qn||  < 1.2e-13;
//   base_q = fl32(1 - m_q), |1 - m_q| <= 2 + 1e-6:                  <= 2^-24 * 2.01  < 1.2e-7;
//   base_q - a_q and B = base_q - a_q - b_q E now reach 2 where 1 - a_q stayed below 1: each of the
//     two fp32 roundings can double, + 2 * 2^-24                                  < 1.2e-7.
//   Sum < 3.7e-7, taken as 5e-7.  (lo = B - A acc itself already ranged over [0, 2].)
// Without a centre base_q = 1.0f exactly and no bit of any plane, workspace value or result changes.
//
// Pipeline (launch_coarse, kind CM_DENSE_Q8): dense_prep_q8 -> f16 sample seed: K1c MINONLY over a
// 1/16 row sample of the f16 plane (per group: min coarse distance), seed = the k-th smallest group
// minimum + K1c's bound E (>= the true k-th distance) -> K1q, the int8 scan: every live + allowed
// row with d~ - E_r <= seed into its (range, query) buffer -> dense_rerank_q8_kernel, three stages:
// kth_up = k-th smallest d~ + E_r over the candidates, tightened to the k-th exact distance of the
// rows at or below it (the pilot bound, at the kernel), and the int8 band = the candidates with
// d~ - E_r <= that bound (it holds every exact top-k row); the f16 band = its rows still certifiable
// after re-scoring from the f16 plane (skipped when only the plane's sample prefix is held); exact
// fp64 re-rank of that band from the fp32 rows ->
// dense_rerank_wide_kernel for the queries whose band exceeds kQBand with complete candidate
// buffers.  A query whose buffer overflows (or that the wide re-rank cannot hold) goes to the exact
// fp32 K1 pass, as K1c's.  K1q-s (kind CM_DENSE_Q8S) is the same with K1s MINONLY as the sample
// pass and dense_q8_stream_kernel as the scan.

// k order inside a 64-k block: lane group g holds the bytes k = 16 g .. 16 g + 15.  Rows and queries
// are packed through the same q8_ge, so the order is exact whatever it is (a k permutation applied
// to both operands leaves every dot product unchanged; tools/mfma_i8_probe.hip).
#ifndef K1Q_RING
#define K1Q_RING 12
#endif
#ifndef K1Q_DBG
#define K1Q_DBG 0  // timing ablations only (tools/build_dense_variant.sh -DK1Q_DBG=<bits>); product: 0
#endif
constexpr int kQDbg = K1Q_DBG;  // 2 no candidate stores | 16 staged entries dropped | 32 no append loop | 64 no staging | 128 no epilogue | 1024 no DMA in the loop | 4096 no MFMA | 8192 L2-resident source
constexpr int kQRing = K1Q_RING;  // LDS ring slots of 8 KiB (one 64 x 128 chunk each)
constexpr int kQCap = 128;        // candidate slots per (range, query)
// the re-rank's capacity (candidates gathered into LDS = int8-band rows) and its workgroup size
// (compile-time A/B knobs; the LDS it needs is 12 B per capacity slot).  4096 (48 KiB + 14 KiB static,
// so three BM25 K2b blocks fit beside it) instead of 8192 (110 KiB): 32.1-32.2k vs 31.9-32.0k q/s in
// the headline step, BM25 search 3.77 vs 3.93 ms (profiles/r06_rerank_ab.txt); the bench's bands stay
// ~1k rows, a wider band (near-duplicate clusters) goes to the wide re-rank as before
#ifndef K1Q_RR
#define K1Q_RR 4096
#endif
#ifndef K1Q_RT
#define K1Q_RT 1024   // 16 waves per query: 4x the fp64 stage's row loads in flight (256 until late round 6:
                      // standalone 10M B = 256 search 2.72 -> 2.52 ms, profiles/r06_rerank_threads_ab.txt)
#endif
constexpr int kQBand = K1Q_RR;       // int8-band rows per query (Gaussian queries at 10M: up to ~3k)
constexpr int kQBand2 = K1Q_RR / 2;  // f16-band rows per query the fp64 stage re-scores (~30 at the bench shape)
constexpr int kQRT = K1Q_RT, kQRW = K1Q_RT / 64;   // re-rank threads / waves per query
constexpr int kQSel = 256;        // rows at or below the band's k-th distance ranked for the output
constexpr int kQMeta = 4;         // LDS slots of 1 KiB for the tiles' row scales + live / allow words
// K1q's LDS budget: ring + metadata slots + staging + counters, in two footprints.  The full 160 KiB
// (the most staging: fewest processing passes) when the scan has the GPU to itself; 131 KiB when the
// caller runs other work beside it (the deferred search of the hybrid step, cm_dense_search_dev_deferred):
// it leaves room for one BM25 block (K2b 28.2 KiB; K2a's one-wave blocks 6.7 KiB each) beside every K1q workgroup, so the
// BM25 stream overlaps the scan on the same CUs instead of waiting for K1q's last workgroup
// (headline step 8.48 -> 8.31 ms with the 256-thread BM25 merge, profiles/r05_lds_ab.txt)
#ifndef K1Q_LDS
#define K1Q_LDS (160 * 1024)
#endif
#ifndef K1Q_LDS_SHARED
#define K1Q_LDS_SHARED (131 * 1024)
#endif
// vmcnt a K1q wave may leave outstanding once chunk y has landed, chunks up to z issued: 2 pieces
// per chunk, plus one tile-metadata DMA right after the pieces of every chunk that starts a tile
// (6 chunks per tile at ld 768).
constexpr int q8_vm_after(int y, int z) {
  int n = 2 * (z - y);
  for (int x = y; x <= z; ++x) n += x % 6 == 0 ? 1 : 0;
  return n;
}

typedef int i32x4q __attribute__((ext_vector_type(4)));

__host__ __device__ inline void q8_ge(int k6, int &g, int &e) {
  g = k6 >> 4;
  e = k6 & 15;
}
__host__ __device__ inline int64_t q8_plane_off(int64_t row, int k, int ld) {
  const int64_t tile = row >> 6;
  const int rr = (int)(row & 63), rt = rr >> 4, j = rr & 15;
  const int c = k >> 7, kk = k & 127, kh = kk >> 6;
  int g, e;
  q8_ge(kk & 63, g, e);
  return (((tile * (ld >> 7) + c) * 8 + rt * 2 + kh) << 10) + ((g * 16 + j) << 4) + e;
}
// query fragments: [16-query tile][chunk][kh][lane][16 bytes]
__host__ __device__ inline int64_t q8_query_off(int64_t q, int k, int ld) {
  const int64_t qt = q >> 4;
  const int j = (int)(q & 15);
  const int c = k >> 7, kk = k & 127, kh = kk >> 6;
  int g, e;
  q8_ge(kk & 63, g, e);
  return (((qt * (ld >> 7) + c) * 2 + kh) << 10) + ((g * 16 + j) << 4) + e;
}

__device__ inline float block256_max(float v, float *red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ inline double block256_sum(double v, double *red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Quantise one vector (ld values xn_of(c), 0 past dim) with one 256-thread block: writes the 8-bit
// codes through put(c, code) and returns {scale, e >= ||xn - scale q8||, n >= ||scale q8||}.
template <typename XN, typename PUT>
__device__ inline float3 q8_quantise(XN xn_of, PUT put, int ld) {
  __shared__ float redf[4];
  __shared__ double redd[4];
  float amax = 0.f;
  for (int c = threadIdx.x; c < ld; c += 256) amax = fmaxf(amax, fabsf(xn_of(c)));
  amax = block256_max(amax, redf);
  const float s = amax > 0.f ? amax / 127.f : 1.f;
  double er = 0.0, nr = 0.0;
  for (int c = threadIdx.x; c < ld; c += 256) {
    const float x = xn_of(c);
    const int q = max(-127, min(127, (int)rintf(x / s)));
    put(c, (int8_t)q);
    const double xt = (double)s * (double)q;  // exact in fp64
    er += ((double)x - xt) * ((double)x - xt);
    nr += xt * xt;
  }
  er = block256_sum(er, redd);
  nr = block256_sum(nr, redd);
  // rounded up: the fp64 sums' error is far below 1e-6 relative
  return make_float3(s, (float)(sqrt(er) * (1.0 + 1e-6)), (float)(sqrt(nr) * (1.0 + 1e-6)));
}

// Row groups.  The scan's per-lane candidate pre-test (below) needs one scale for the 16 rows a
// lane holds: group G = (tile T, lane group g) = rows 64 T + 16 rt + 4 g + r (rt, r = 0..3).  Every
// row of a group is quantised with the group's scale S = max over its rows of max|xn| / 127
// (+16 % quantisation error against a per-row scale at 768-d, so ~8 % on the bound E), rmeta[row] =
// {S, e_r} with the row's own e_r >= ||xn - S q8|| (fp64, rounded up).  An upsert re-quantises the
// groups of the rows it wrote (dense_q8_group_kernel, one block per group).
__host__ __device__ inline int64_t q8_group_of(int64_t row) { return (row >> 6) * 4 + ((row >> 2) & 3); }
__host__ __device__ inline int64_t q8_group_row(int64_t G, int i) {   // row i (0..15) of group G
  return (G >> 2) * 64 + 16 * (i >> 2) + 4 * (G & 3) + (i & 3);
}
__global__ void __launch_bounds__(256) dense_q8_group_kernel(const float *__restrict__ C, const float *__restrict__ invc,
                                                             const float *__restrict__ mu,
                                                             const uint32_t *__restrict__ live,
                                                             const int64_t *__restrict__ groups, int64_t g0, int64_t ng,
                                                             int dim, int ld, int8_t *__restrict__ Xq,
                                                             float2 *__restrict__ rmeta, uint32_t *__restrict__ rnorm) {
  const int64_t gi = blockIdx.x;
  if (gi >= ng) return;
  const int64_t G = groups ? groups[gi] : g0 + gi;
  const int i = threadIdx.x >> 4, l = threadIdx.x & 15;   // 16 threads per row
  const int64_t r = q8_group_row(G, i);
  const float inv = invc[r];
  const float *crow = C + r * ld;
  auto xn_of = [&](int c) { return c < dim ? crow[c] * inv : 0.f; };  // == the f16 plane's xn
  // the quantised vector: xn, or xn - mu under a centre (mu: ld floats, 0 past dim; nullptr = none)
  auto y_of = [&](int c) { return mu ? __fsub_rn(xn_of(c), mu[c]) : xn_of(c); };
  __shared__ float redf[4];
  float amax = 0.f;
  for (int c = l; c < ld; c += 16) amax = fmaxf(amax, fabsf(y_of(c)));
  // centred: an all-zero row (never written, truncated, a zero vector) keeps code 0 and stays out of
  // the group's scale; live, it gets the honest bound e_r = ||mu||; dead (a hole: it can come to
  // life only through an upsert, which re-quantises its group), e_r = 0 -- the scans take the
  // largest e_r of a lane's 16 rows for all of them, so a hole's ||mu|| would make candidates of its
  // 15 group mates in every search.  live == nullptr: every row counts as live (the compaction's
  // moved rows, whose bits are set after this kernel).
  bool zero = false, dead = false;
  if (mu) {   // block-uniform
    float xmax = 0.f;
    for (int c = l; c < ld; c += 16) xmax = fmaxf(xmax, fabsf(xn_of(c)));
    for (int o = 8; o > 0; o >>= 1) xmax = fmaxf(xmax, __shfl_xor(xmax, o));
    zero = xmax == 0.f;
    dead = zero && live && !((live[r >> 5] >> (r & 31)) & 1u);
    if (zero) amax = 0.f;
  }
  amax = block256_max(amax, redf);
  const float s = amax > 0.f ? amax / 127.f : 1.f;
  double er = 0.0, nr = 0.0;
  for (int c = l; c < ld; c += 16) {
    const float x = y_of(c);
    const int q = zero ? 0 : max(-127, min(127, (int)rintf(x / s)));
    Xq[q8_plane_off(r, c, ld)] = (int8_t)q;
    const double xt = (double)s * (double)q;  // exact in fp64
    const double d = zero ? (dead ? 0.0 : (double)mu[c]) : (double)x - xt;   // zero row: d~ = base_q is off by mu.qn
    er += d * d;
    nr += xt * xt;
  }
  for (int o = 8; o > 0; o >>= 1) {
    er += __shfl_xor(er, o);
    nr += __shfl_xor(nr, o);
  }
  if (l == 0) {   // rounded up: the fp64 sums' error is far below 1e-6 relative
    rmeta[r] = make_float2(s, (float)(sqrt(er) * (1.0 + 1e-6)));
    atomicMax(&rnorm[2], __float_as_uint((float)(sqrt(nr) * (1.0 + 1e-6))));
  }
}

// Queries: qn = q / (||q|| + 1e-30) in fp32 (dense_prep_planes' normalisation), its codes in the
// fragment layout, and qsc = {s_q, a_q, b_q, ||q||}: E_r = a_q + b_q e_r with
// a_q = max||x~|| e_q + 4e-6 (+ 5e-7 under a centre: the header's derivation) and b_q = ||qn|| (both
// rounded up); qbase = base_q = fl32(1 - mu.qn), 1.0f without a centre (mu == nullptr).  Padded
// queries (>= nq): zeros (base 1).
__global__ void __launch_bounds__(256) dense_prep_q8(const float *__restrict__ q, int nq, int dim, int ld,
                                                     int8_t *__restrict__ Qq, float4 *__restrict__ qsc,
                                                     const uint32_t *__restrict__ rnorm,
                                                     const float *__restrict__ mu, float *__restrict__ qbase) {
  const int qi = blockIdx.x;
  const float *src = q + (int64_t)qi * dim;
  __shared__ double redd[4];
  double t = 0.0;
  float tf = 0.f;
  for (int i = threadIdx.x; i < dim; i += 256) {
    const float v = qi < nq ? src[i] : 0.f;
    tf += v * v;
  }
  __shared__ float redf[4];
  for (int o = 32; o > 0; o >>= 1) tf += __shfl_xor(tf, o);
  if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = tf;
  __syncthreads();
  const float tt = (redf[0] + redf[1]) + (redf[2] + redf[3]);
  const float inv = 1.0f / (sqrtf(tt) + 1e-30f);
  auto xn_of = [&](int c) { return (qi < nq && c < dim) ? src[c] * inv : 0.f; };
  const float3 m = q8_quantise(xn_of, [&](int c, int8_t v) { Qq[q8_query_off(qi, c, ld)] = v; }, ld);
  for (int c = threadIdx.x; c < ld; c += 256) {
    const double x = (double)xn_of(c);
    t += x * x;
  }
  t = block256_sum(t, redd);
  double mq = 0.0;   // mu.qn
  if (mu) {          // uniform
    for (int c = threadIdx.x; c < ld; c += 256) mq += (double)mu[c] * (double)xn_of(c);
    mq = block256_sum(mq, redd);
  }
  if (threadIdx.x == 0) {
    const double nmax = (double)__uint_as_float(rnorm[2]);
    const float a = (float)(nmax * (double)m.y * (1.0 + 1e-6) + (mu ? 4e-6 + 5e-7 : 4e-6));
    const float b = (float)(sqrt(t) * (1.0 + 1e-6));
    qsc[qi] = make_float4(m.x, a, b, sqrtf(tt));
    qbase[qi] = mu ? (float)(1.0 - mq) : 1.0f;
  }
}

// K1q scan (ld = 768: 6 chunks of 128 k per 64-row tile).  One workgroup of 4 waves per (pass of
// 256 queries, row range), one per CU; wave w owns queries 64 w .. + 63 of the pass, their int8
// fragments resident in AGPRs (6 chunks x 2 k-halves x 4 q-tiles = 192 registers), so the LDS is
// the corpus ring (kQRing slots of 8 KiB, LDS-DMA, counted vmcnt + one barrier per chunk) plus the
// tiles' metadata slots and the candidate staging.  Per chunk: 32 v_mfma_i32_16x16x64_i8 per wave;
// the next chunk's fragments are read (double buffer) between the two halves.
//
// Epilogue per tile (v6).  Lane (g, j) holds the products of query qt * 16 + j with the 16 rows of
// its row group (16 rt + 4 g + r), which share one scale S (dense_q8_group_kernel).  With E = the
// group's largest e_r, every row's bounds d~ - E_r >= lo_r = B - A acc_r and d~ + E_r <= lo_r + W,
// A = s_q S, B = base_q - a_q - b_q E, W = 2 (a_q + b_q E) + 1e-6 (E >= e_r: valid, ~5 % looser than
// the row's own e_r, which is nearly the group's under a shared scale), so one integer max3 tree
// per (lane, q-tile) decides the whole lane:
// no row of the lane passes lo_r <= seed unless B - A max acc <= seed (the same fp32 expression,
// monotone in acc: exact, no margin).
// That replaces ~4 VALU issues per (row, query) pair (v4/v5: the tests alone cost 0.5-0.9 ms of a
// 1.15 ms scan, profiles/r04b_k1q_abl.txt).  A lane that passes stages one 96-B entry -- query,
// live bits, first row, A, B, W, seed, its 16 raw products -- in the wave's LDS area; when the area
// is full (and at the end) the wave processes the entries one per lane (SIMD-efficient: 64 entries
// per pass instead of one ballot per row position): per row lo <= seed -> slot from the query's LDS
// counter, key (f32_order(lo), row) and up = lo + W stored into the (range, query) buffer.  No global
// loads anywhere in the loop (they would drain the LDS-DMA ring); the stores cost one counted-wait
// over-wait per processing pass.
constexpr int kQDumpB = 96;     // bytes per staged entry
// ring slots of the full-LDS form (A/B knob; the shared 131 KiB form keeps kQRing: its staging needs the rest)
#ifndef K1Q_RING_FULL
#define K1Q_RING_FULL K1Q_RING
#endif
template <int LDS>
struct K1qLds {
  static constexpr int ring = LDS >= 160 * 1024 ? K1Q_RING_FULL : kQRing;
  static constexpr int stage_e = (LDS - ring * 8192 - kQMeta * 1024 - 1024) / (4 * kQDumpB);  // staging entries per wave
  static constexpr int cnt_off = ring * 8192 + kQMeta * 1024 + 4 * stage_e * kQDumpB;         // per-query counters (4 x 64)
  static constexpr int total = cnt_off + 1024;
  static_assert(total <= 160 * 1024 && stage_e >= 64, "K1q LDS: ring + metadata + staging + counters");
};
constexpr int kQLds = K1qLds<K1Q_LDS>::total, kQLdsShared = K1qLds<K1Q_LDS_SHARED>::total;
template <int LDS = K1Q_LDS>
__global__ void __launch_bounds__(256, 1)
    dense_q8_scan_kernel(const int8_t *__restrict__ Xq, const float2 *__restrict__ rmeta,
                         const uint32_t *__restrict__ live, const uint32_t *__restrict__ allow, int64_t n_words,
                         const int8_t *__restrict__ Qq, const float4 *__restrict__ qsc,
                         const float *__restrict__ qbase, int nq,
                         const float *__restrict__ seed, int64_t rows_per_wg, int64_t rows_end, int n_wg,
                         uint64_t *__restrict__ out_keys, float *__restrict__ out_up,
                         uint32_t *__restrict__ out_cnt) {
  constexpr int KC = 6, QT = 4, PCS = 2, RING = K1qLds<LDS>::ring;
  constexpr int kQStageE = K1qLds<LDS>::stage_e, kQCntOff = K1qLds<LDS>::cnt_off;
  static_assert(RING > KC + 1, "the tile's row scales must be younger than every chunk the tile waits for");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wg = blockIdx.x % n_wg, qp = blockIdx.x / n_wg;
  const int64_t r_begin = (int64_t)wg * rows_per_wg;
  const int64_t r_end = min(r_begin + rows_per_wg, rows_end);
  const int ntiles = r_begin < r_end ? (int)((r_end - r_begin) >> 6) : 0;
  const int total = ntiles * KC;
  const int qc0 = wave * 64;                       // the wave's first query within the pass
  const int64_t qt0 = ((int64_t)qp * kBQPass + qc0) >> 4;
  i32x4q qf[KC][2][QT];
#pragma unroll
  for (int c = 0; c < KC; ++c)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
        qf[c][kh][qt] = *reinterpret_cast<const i32x4q *>(Qq + ((((qt0 + qt) * KC + c) * 2 + kh) << 10) + lane * 16);
  // resident in AGPRs, read there by the MFMAs (pinned after every load is in flight: one pin per
  // load would serialise the 48 loads behind 48 vmcnt(0) waits)
#pragma unroll
  for (int c = 0; c < KC; ++c)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) asm volatile("" : "+a"(qf[c][kh][qt]));
  // per q-tile constants of the lane's query: s_q, base_q - a_q, a_q, b_q, seed (-inf when padded)
  float sq[QT], oaq[QT], aq[QT], bq[QT], sdq[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qq = qp * kBQPass + qc0 + qt * 16 + j;
    const float4 v = qsc[qq];
    sq[qt] = v.x;
    aq[qt] = v.y;
    oaq[qt] = qbase[qq] - v.y;   // base_q - a_q (base_q = 1.0f without a centre)
    bq[qt] = v.z;
    sdq[qt] = qq < nq ? seed[qq] : -__builtin_inff();
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), seen by the compiler's wait tracking
  const __attribute__((address_space(1))) unsigned char *Xb = (const __attribute__((address_space(1))) unsigned char *)Xq;
  const int64_t cb = (r_begin >> 6) * KC;
  const uint32_t *allw = allow ? allow : live;
  unsigned char *meta = lds + RING * 8192;
  // tile T's metadata into slot T % kQMeta: waves 0-1 its 64 rmeta entries (512 B), wave 2 the live
  // and allow words of its rows (dwords 128..131), wave 3 a copy of rmeta into the slot's unused
  // tail (every wave issues exactly one DMA, so the vmcnt bookkeeping is wave-independent)
  auto issue_meta = [&](int T) __attribute__((always_inline)) {
    const int Tc = min(T, ntiles - 1);
    const int64_t row0 = r_begin + (int64_t)Tc * 64;
    const unsigned char *src;
    if (wave == 2) {
      const int64_t wi = (row0 >> 5) + (lane & 1);
      const int64_t wc = wi < n_words ? wi : n_words - 1;
      src = reinterpret_cast<const unsigned char *>((lane & 2) ? allw + wc : live + wc);
    } else {
      src = reinterpret_cast<const unsigned char *>(rmeta + row0) + (wave & 1) * 256 + lane * 4;
    }
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)(meta + (T % kQMeta) * 1024 + wave * 256),
                                     4, 0, 0);
  };
  auto issue_piece = [&](int gc, int i) __attribute__((always_inline)) {
    int gl = min(gc, total - 1);                     // clamped: one control path past the end
    if (kQDbg & 8192) gl &= 15;
    const int o = 4 * i + wave;
    __builtin_amdgcn_global_load_lds(Xb + (((cb + gl) * 8 + o) << 10) + lane * 16,
                                     (__attribute__((address_space(3))) void *)(lds + (gc % RING) * 8192 + o * 1024),
                                     16, 0, kK1cAux);
  };
  auto issue = [&](int gc, bool tile_start) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PCS; ++i) issue_piece(gc, i);
    if (tile_start) issue_meta(gc / KC);
  };
  auto frag = [&](int gc, int rt, int kh) -> i32x4q {
    return *reinterpret_cast<const i32x4q *>(lds + (gc % RING) * 8192 + (rt * 2 + kh) * 1024 + lane * 16);
  };
  // this wave's staging (kQStageE entries of 96 B) and its 64 queries' candidate counters,
  // written and read through inline asm (plain LDS accesses here would make the compiler drain the
  // ring first)
  const uint32_t stg = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)(
      lds + RING * 8192 + kQMeta * 1024 + wave * kQStageE * kQDumpB);
  const uint32_t cnt_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)(
      lds + kQCntOff + wave * 256);
  const int64_t qbuf0 = ((int64_t)qp * n_wg + wg) * kBQPass + qc0;   // the wave's first (range, query) buffer
  uint32_t nst = 0, dbg_sink = 0;
  // exact per-row tests of n staged entries, one entry per lane, and the appends
  auto process = [&](uint32_t n) __attribute__((always_inline)) -> uint32_t {
    if (kQDbg & 16) return 0u;                           // ablation: staged entries dropped
    for (uint32_t e = lane; e < n; e += 64) {
      const uint32_t a0 = stg + e * kQDumpB;
      i32x4q h0, h1, av0, av1, av2, av3;
      asm volatile("ds_read_b128 %0, %6\n\t"
                   "ds_read_b128 %1, %6 offset:16\n\t"
                   "ds_read_b128 %2, %6 offset:32\n\t"
                   "ds_read_b128 %3, %6 offset:48\n\t"
                   "ds_read_b128 %4, %6 offset:64\n\t"
                   "ds_read_b128 %5, %6 offset:80\n\t"
                   "s_waitcnt lgkmcnt(0)"
                   : "=&v"(h0), "=&v"(h1), "=&v"(av0), "=&v"(av1), "=&v"(av2), "=&v"(av3)
                   : "v"(a0)
                   : "memory");
      const uint32_t ql = (uint32_t)h0[0] & 63u, live16 = (uint32_t)h0[0] >> 16;
      const int64_t rb = (int64_t)(uint32_t)h0[1];
      const float A = __int_as_float(h0[2]), B = __int_as_float(h0[3]);
      const float W = __int_as_float(h1[0]), sd = __int_as_float(h1[1]);
      const i32x4q av[4] = {av0, av1, av2, av3};
      uint32_t hm = 0;                                   // the entry's passing rows (branch-free)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        hm |= (fmaf(-A, (float)av[i >> 2][i & 3], B) <= sd ? 1u : 0u) << i;
      hm &= live16;
      // one counter round trip per entry, then the lane's few hits (their products re-read from
      // the staged entry: a per-lane register index would be a select tree)
      uint32_t slot;
      asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
                   : "=v"(slot) : "v"(cnt_lds + ql * 4), "v"((kQDbg & (2 | 32)) ? 0u : (uint32_t)__popc(hm))
                   : "memory");   // (ablations 2 / 32 write no candidate: they count none either)
      const int64_t ob = (qbuf0 + ql) * kQCap;
      if (kQDbg & 32) hm = 0;                             // ablation: no append loop
      while (hm) {
        const int i = __builtin_ctz(hm);
        hm &= hm - 1u;
        int av_i;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(av_i) : "v"(a0 + 32 + 4 * i) : "memory");
        if (slot < (uint32_t)kQCap && !(kQDbg & 2)) {    // (ablation 2: no global stores)
          const float lo = fmaf(-A, (float)av_i, B);
          const int64_t row = rb + 16 * (i >> 2) + (i & 3);
          out_keys[ob + slot] = ((uint64_t)f32_order(lo) << 32) | (uint64_t)(uint32_t)row;
          out_up[ob + slot] = lo + W;
        }
        ++slot;
      }
    }
    return 0u;
  };
  reinterpret_cast<uint32_t *>(lds + kQCntOff)[tid] = 0u;   // the 4 waves' counters
  i32x4q acc[4][QT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[rt][qt] = i32x4q{0, 0, 0, 0};

  if (total > 0) {
#pragma unroll
    for (int p = 0; p < RING; ++p) issue(p, p % KC == 0);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(q8_vm_after(0, RING - 1)) : "memory");
    __builtin_amdgcn_s_barrier();
    // Interleaved chunk schedule (K1c's, dense_coarse_scan_kernel): with one wave per SIMD nothing
    // hides a non-MFMA instruction but the MFMA issued before it, so every LDS read, the counted
    // wait, the barrier and the DMA pieces of a chunk are threaded one per MFMA gap
    // (sched_barrier-fenced).  The blocked form (16 MFMAs | wait, barrier, DMA, 8 reads | 16 MFMAs)
    // ran the MFMA loop at ~47 % of its issue rate (no-DMA ablation 2.0 ms at 10M x B = 256).
    //   half 1 (row tiles 0-1, fragments read half a chunk earlier): gaps 0-3 read row fragments
    //     2-3 of chunk gc (its slot certified by the previous chunk's barrier); gap W0 waits for
    //     chunk gc+1 (the younger chunks / metadata DMAs may stay in flight: a static count per cc)
    //     and the own LDS reads, then the barrier (chunk gc+1 visible, every read of slot gc
    //     retired); the next gaps issue chunk gc + RING into slot gc (+ its tile's metadata);
    //   half 2 (row tiles 2-3): gaps 0-3 read row fragments 0-1 of chunk gc+1.
    // Tile t's metadata rides with chunk 6t, so it has landed (in-order vmcnt) and is visible once
    // step 5 of tile t has passed its barrier.
    i32x4q xf[4][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) xf[rt][kh] = frag(0, rt, kh);
    constexpr int W0 = 16 - PCS - 2;
    // The tile epilogue's inputs, gathered in the MFMA gaps of the tile's last chunk (its second half)
    // instead of after it: the tile's metadata (visible since that chunk's barrier) -- the live /
    // allow words, the lane group's scale S and its 16 rows' e_r -- and the integer maxima of row
    // tiles 0-2 per q-tile (final by then); the epilogue folds in row tile 3.  With one wave per SIMD
    // the serial epilogue (9 LDS reads + their wait, ~60 max operations) cost every tile ~10 % of its
    // MFMA time; here the VALU work fills MFMA issue gaps.  Same values: the maxima over the same 16
    // products, E over the same e_r (non-negative floats order as their bits).
    const uint32_t meta_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)meta;
    int pm[QT];
    uint32_t eu = 0u, s_bits = 0u;   // (eu restarts at gap 11 of every tile)
    i32x4q wdv;
    uint64_t ev[8];
    auto tail = [&](int m, int t) __attribute__((always_inline)) {
      const uint32_t mb = meta_lds + (t % kQMeta) * 1024;
      if (m == 0) {
        asm volatile("ds_read_b128 %0, %10 offset:512\n\t"
                     "ds_read_b32 %1, %11\n\t"
                     "ds_read2_b32 %2, %11 offset0:1 offset1:3\n\t"
                     "ds_read2_b32 %3, %11 offset0:5 offset1:7\n\t"
                     "ds_read2_b32 %4, %11 offset0:33 offset1:35\n\t"
                     "ds_read2_b32 %5, %11 offset0:37 offset1:39\n\t"
                     "ds_read2_b32 %6, %11 offset0:65 offset1:67\n\t"
                     "ds_read2_b32 %7, %11 offset0:69 offset1:71\n\t"
                     "ds_read2_b32 %8, %11 offset0:97 offset1:99\n\t"
                     "ds_read2_b32 %9, %11 offset0:101 offset1:103"
                     : "=&v"(wdv), "=&v"(s_bits), "=&v"(ev[0]), "=&v"(ev[1]), "=&v"(ev[2]), "=&v"(ev[3]),
                       "=&v"(ev[4]), "=&v"(ev[5]), "=&v"(ev[6]), "=&v"(ev[7])
                     : "v"(mb), "v"(mb + 32 * g)
                     : "memory");
      }
      if (m >= 3 && m <= 10) {   // row tiles 0-1: two gaps per q-tile
        const int q = (m - 3) >> 1;
        if (((m - 3) & 1) == 0) {
          pm[q] = max(max(acc[0][q][0], acc[0][q][1]), acc[0][q][2]);
          pm[q] = max(max(pm[q], acc[0][q][3]), acc[1][q][0]);
        } else {
          pm[q] = max(max(pm[q], acc[1][q][1]), acc[1][q][2]);
          pm[q] = max(pm[q], acc[1][q][3]);
        }
        asm volatile("" : "+v"(pm[q]));   // computed here, in this gap (not sunk into the epilogue)
      }
      if (m == 11) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (m >= 11 && m <= 14) {  // E: e_r of rows 2 h, 2 h + 1 of records 2 (m - 11), + 1
        const int k0 = 2 * (m - 11);
        eu = max(max(m == 11 ? 0u : eu, (uint32_t)ev[k0]), (uint32_t)(ev[k0] >> 32));   // per tile
        eu = max(max(eu, (uint32_t)ev[k0 + 1]), (uint32_t)(ev[k0 + 1] >> 32));
        asm volatile("" : "+v"(eu));
      }
      if (m >= 12) {             // row tile 2 (final since gap 4 + q)
        const int q = m - 12;
        pm[q] = max(max(pm[q], acc[2][q][0]), acc[2][q][1]);
        pm[q] = max(max(pm[q], acc[2][q][2]), acc[2][q][3]);
        asm volatile("" : "+v"(pm[q]));
      }
    };
#define K1Q_STEP(gcv, cc)                                                                                             \
  do {                                                                                                                \
    _Pragma("unroll") for (int m = 0; m < 16; ++m) {                                                                  \
      const int rt = m >> 3, kh = (m >> 2) & 1, qt = m & 3;                                                           \
      if (!(kQDbg & 4096))                                                                                            \
        acc[rt][qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[rt][kh], qf[cc][kh][qt], acc[rt][qt], 0, 0, 0);        \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
      if (m < 4) xf[2 + (m >> 1)][m & 1] = frag((gcv), 2 + (m >> 1), m & 1);                                          \
      if (m == W0) {                                                                                                  \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(q8_vm_after((cc) + 1, (cc) + RING - 1)) : "memory");      \
        __builtin_amdgcn_s_barrier();                                                                                 \
      }                                                                                                               \
      if (!(kQDbg & 1024) && m > W0 && m <= W0 + PCS) issue_piece((gcv) + RING, m - W0 - 1);                          \
      if (!(kQDbg & 1024) && m == W0 + PCS + 1 && ((cc) + RING) % KC == 0) issue_meta(((gcv) + RING) / KC);           \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
    }                                                                                                                 \
    _Pragma("unroll") for (int m = 0; m < 16; ++m) {                                                                  \
      const int rt = 2 + (m >> 3), kh = (m >> 2) & 1, qt = m & 3;                                                     \
      if (!(kQDbg & 4096))                                                                                            \
        acc[rt][qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[rt][kh], qf[cc][kh][qt], acc[rt][qt], 0, 0, 0);        \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
      if (m < 4) xf[m >> 1][m & 1] = frag((gcv) + 1, m >> 1, m & 1);                                                  \
      if ((cc) == KC - 1 && !(kQDbg & 128)) tail(m, t);                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
    }                                                                                                                 \
  } while (0)
    for (int t = 0; t < ntiles; ++t) {
      const int64_t row0 = r_begin + (int64_t)t * 64;
      const int gc0 = t * KC;
      K1Q_STEP(gc0 + 0, 0);
      K1Q_STEP(gc0 + 1, 1);
      K1Q_STEP(gc0 + 2, 2);
      K1Q_STEP(gc0 + 3, 3);
      K1Q_STEP(gc0 + 4, 4);
      K1Q_STEP(gc0 + 5, 5);
      // ---- epilogue
      if (!(kQDbg & 128)) {
      const int64_t w0 = row0 >> 5;                 // wdv = live0, live1, allow0, allow1
      const uint32_t m0 = w0 < n_words ? ((uint32_t)wdv[0] & (uint32_t)wdv[2]) : 0u;
      const uint32_t m1 = w0 + 1 < n_words ? ((uint32_t)wdv[1] & (uint32_t)wdv[3]) : 0u;
      const bool full = (m0 & m1) == 0xffffffffu;   // wave-uniform (every lane read the same words)
      const float S = __uint_as_float(s_bits);      // the lane's row group: one scale
      const float E = __uint_as_float(eu);          // and the largest e_r of its rows
      int amax[QT];
      uint32_t live16 = 0xffffu;
      if (full) {                                    // row tiles 0-2 folded in the last chunk's gaps
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          const int m = max(max(pm[qt], acc[3][qt][0]), acc[3][qt][1]);
          amax[qt] = max(max(m, acc[3][qt][2]), acc[3][qt][3]);
        }
      } else {                                       // dead / filtered rows leave the maximum
        live16 = lane_live16(((uint64_t)m1 << 32) | m0, g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          int m = INT32_MIN;
#pragma unroll
          for (int i = 0; i < 16; ++i) m = max(m, ((live16 >> i) & 1u) ? acc[i >> 2][qt][i & 3] : INT32_MIN);
          amax[qt] = m;
        }
      }
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const float A = sq[qt] * S, B = fmaf(-bq[qt], E, oaq[qt]);
        const float W = 2.0f * fmaf(bq[qt], E, aq[qt]) + 1e-6f;
        const float lmin = fmaf(-A, (float)amax[qt], B);    // the lane's smallest lo_r
        const bool pass = lmin <= sdq[qt] && amax[qt] != INT32_MIN;
        const uint64_t P = __ballot(pass);
        if (kQDbg & 64) {                            // ablation: pre-test kept alive, nothing staged
          dbg_sink += (uint32_t)__popcll(P);
          continue;
        }
        if (P == 0) continue;                        // wave-uniform
        const uint32_t np = (uint32_t)__popcll(P);
        if (nst + np > (uint32_t)kQStageE) nst = process(nst);
        if (pass) {
          const uint32_t pos = nst + __builtin_amdgcn_mbcnt_hi((uint32_t)(P >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)P, 0u));
          const uint32_t a = stg + pos * kQDumpB;
          const i32x4q h0 = {(int)((uint32_t)(qt * 16 + j) | (live16 << 16)), (int)(uint32_t)(row0 + 4 * g),
                             __float_as_int(A), __float_as_int(B)};
          const i32x4q h1 = {__float_as_int(W), __float_as_int(sdq[qt]), 0, 0};
          asm volatile("ds_write_b128 %0, %1\n\t"
                       "ds_write_b128 %0, %2 offset:16\n\t"
                       "ds_write_b128 %0, %3 offset:32\n\t"
                       "ds_write_b128 %0, %4 offset:48\n\t"
                       "ds_write_b128 %0, %5 offset:64\n\t"
                       "ds_write_b128 %0, %6 offset:80"
                       ::"v"(a), "v"(h0), "v"(h1), "v"(acc[0][qt]), "v"(acc[1][qt]), "v"(acc[2][qt]), "v"(acc[3][qt])
                       : "memory");
        }
        nst += np;
      }
      } else {  // ablation 128: a trivial epilogue keeps the MFMAs alive (the loop's own cost)
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) dbg_sink += (uint32_t)acc[rt][qt][0];
      }  // !(kQDbg & 128)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[rt][qt] = i32x4q{0, 0, 0, 0};
    }
#undef K1Q_STEP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // clamped tail DMAs land before the LDS is released
    if (nst) nst = process(nst);
  }
  uint32_t c;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(c) : "v"(cnt_lds + lane * 4) : "memory");
  if ((kQDbg & (64 | 128)) && dbg_sink == 0x7fffffffu) c = 0u;   // keeps the ablations' work observable
  out_cnt[qbuf0 + lane] = c;
}

// K1q-s: the int8 scan for nq <= kSQ queries (single queries and small batches: north_star's
// HBM-bound C2', SURVEY §8d).  K1s's shape over K1q's plane: every wave is an independent stream
// ("virtual group" vg) over a contiguous run of 64-row tiles, the plane's 1 KiB fragment blocks
// loaded straight into a register ring of R chunks (R - 1 in flight, non-temporal: read once) -- no
// LDS, no barrier, no cross-wave hand-off -- and the <= 32 queries' int8 fragments resident in
// AGPRs.  At 16-32 queries the wave is HBM-bound (8-16 i8 MFMAs per 8 KiB chunk), so the 256-slot
// MFMA passes, LDS ring and staging of the batched K1q are pure overhead here.  Per tile, K1q's
// per-lane pre-test: the lane's 16 rows share one scale S, E = their largest e_r, one integer max
// tree per (lane, q-tile) decides whether any row can pass lo <= seed (exact: lo is monotone in
// acc); the few passing lanes test their rows and append (f32_order(lo), row) and up = lo + W to
// the (vg, query) buffer, slots from the running count all four lanes g of query j keep (a prefix
// of the lanes' hit counts, no atomics).  The tile's rmeta, live and allow words are loaded at the
// top of the tile and consumed by its epilogue KC chunks later.  Output layout = K1q's with one
// pass of kSQ queries and n_wg = n_vg, so dense_rerank_q8_kernel certifies and re-ranks it
// unchanged (the same keys, bounds and fp64 distances as the batched K1q).
//
// KC = 128-k chunks per 64-row tile: 6 (ld 768), 8 (ld 1024, dims 897-1024) or 3 (ld 384, below).
// At ld 1024 this kernel
// is the scan of every batch size: a batch above kSQ queries is launched once per kSQ queries on the
// pass's offsets into the fragments, constants, seeds and [pass][group][qs] buffers (launch_coarse),
// so it streams the plane once per pass; a resident-query batched scan would need all 256 AGPRs for
// 256 queries' fragments (KC x 2 x 4 x 4 x 2).  Registers at KC = 8: query fragments KC x 2 x QT x 4 =
// 64 QT AGPRs, accumulators 16 QT, the ring 32 R, the tile's metadata 34.  Resource report (gfx950,
// one wave per SIMD, no scratch in any of them):
//     <QT, R, KC>   VGPRs  AGPRs            <QT, R, KC>   VGPRs  AGPRs
//     <1, 4, 6>      254     48             <2, 4, 6>      256    107     (the ld 768 product)
//     <1, 4, 8>      256     65             <2, 4, 8>      256    155
//     <1, 3, 8>      198     64             <2, 3, 8>      214    128
//     <1, 2, 8>      168     64 (2 waves)   <2, 2, 8>      208    128
// R = 4 for both KC = 8 instances (K1QS_RING8), as at KC = 6: three chunks = 24 KiB per wave, 96 KiB
// per CU in flight, against 64 KiB at R = 3 -- 8 TB/s x ~2 us over 256 CUs wants ~64 KiB per CU, so
// R = 3 has no margin; R = 4 divides KC (TU = 1: one tile of code, where R = 3 unrolls three) and the
// AGPRs above the fragments' 64 QT (1 and 27) are values the allocator parks there instead of
// spilling, as the KC = 6 product does (11 at QT = 2).
//
// KC = 3 (ld 384, dims 257-384): the automatic scan up to kSQ queries, and in passes when forced
// (dense_kind).  Query fragments 3 x 2 x QT x 4 = 24 QT AGPRs.  TU = R / gcd(R, 3), so the ring also
// sets how many tiles of code are unrolled.  Candidates (no scratch, no LDS in any; in flight = R - 1
// chunks of 8 KiB per wave, x 4 per CU):
//     <QT, R, KC>   VGPRs  AGPRs  waves/SIMD    <QT, R, KC>   VGPRs  AGPRs    TU   in flight per wave
//     <1, 3, 3>      184     24      2          <2, 3, 3>      212     48      1    16 KiB
//     <1, 4, 3>      222     24      2          <2, 4, 3>      254     48      4    24 KiB
//     <1, 6, 3>      256     47      1          <2, 6, 3>      256     99      2    40 KiB
//     (<., 2, 3> 158 / 186 VGPRs and <., 5, 3> 256 + 77 / 123 AGPRs were compiled and not run)
// Scan kernel alone at 1M x 384, k = 24, ms at 1 / 16 / 32 queries and two passes for 64
// (profiles/dense_dim384.txt): R = 3 0.067 / 0.072 / 0.076 / 0.149, R = 4 0.067 / 0.073 / 0.078 / 0.154,
// R = 6 0.067 / 0.073 / 0.081 / 0.156.  A deeper ring buys nothing here -- a tile is 24 KiB, so the 16 KiB
// of R = 3 already cover two thirds of the next tile while this one's epilogue runs, and the stream is
// shorter than at KC = 8, where R = 3 lost 6 % -- so K1QS_RING3 = 3: equal or ahead at every batch size,
// one tile of code, the fewest registers.
#ifndef K1QS_RING
#define K1QS_RING 4
#endif
#ifndef K1QS_RING8
#define K1QS_RING8 4
#endif
#ifndef K1QS_RING3
#define K1QS_RING3 3
#endif
constexpr int cgcd(int a, int b) { return b == 0 ? a : cgcd(b, a % b); }
template <int QT, int R, int KC>
__global__ void __launch_bounds__(256, 1)
    dense_q8_stream_kernel(const int8_t *__restrict__ Xq, const float2 *__restrict__ rmeta,
                           const uint32_t *__restrict__ live, const uint32_t *__restrict__ allow, int64_t n_words,
                           const int8_t *__restrict__ Qq, const float4 *__restrict__ qsc,
                           const float *__restrict__ qbase, int nq,
                           const float *__restrict__ seed, int64_t rows_per_vg, int64_t rows_end, int n_vg,
                           uint64_t *__restrict__ out_keys, float *__restrict__ out_up,
                           uint32_t *__restrict__ out_cnt) {
  static_assert(KC == 3 || KC == 6 || KC == 8, "K1q-s: 128-k chunks per 64-row tile, ld 384, 768 or 1024");
  constexpr int TU = R / cgcd(R, KC);       // tiles per unrolled iteration: static ring slots
  const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int vg = blockIdx.x * 4 + wave;
  if (vg >= n_vg) return;                   // wave-uniform; the kernel has no barriers
  const int64_t r_begin = (int64_t)vg * rows_per_vg;
  const int64_t r_end = min(r_begin + rows_per_vg, rows_end);
  const int ntiles = r_begin < r_end ? (int)((r_end - r_begin) >> 6) : 0;
  const int total = ntiles * KC;

  float sq[QT], oaq[QT], aq[QT], bq[QT], sdq[QT];
  uint32_t qcnt[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qq = qt * 16 + j;
    const float4 v = qsc[qq];
    sq[qt] = v.x;
    aq[qt] = v.y;
    oaq[qt] = qbase[qq] - v.y;   // base_q - a_q (base_q = 1.0f without a centre)
    bq[qt] = v.z;
    sdq[qt] = qq < nq ? seed[qq] : -__builtin_inff();
    qcnt[qt] = 0u;
  }
  i32x4q qf[KC][2][QT];
#pragma unroll
  for (int c = 0; c < KC; ++c)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
        qf[c][kh][qt] = *reinterpret_cast<const i32x4q *>(Qq + (((qt * KC + c) * 2 + kh) << 10) + lane * 16);
#pragma unroll
  for (int c = 0; c < KC; ++c)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) asm volatile("" : "+a"(qf[c][kh][qt]));
  i32x4q acc[4][QT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) acc[rt][qt] = i32x4q{0, 0, 0, 0};

  if (total > 0) {
    const i32x4q *Xv = reinterpret_cast<const i32x4q *>(Xq);
    const int64_t chunk0 = (r_begin >> 6) * KC;   // the wave's chunks are contiguous
    i32x4q xb[R][8];
    auto load = [&](i32x4q (&b)[8], int gc) __attribute__((always_inline)) {
      const int gl = min(gc, total - 1);          // clamped: one control path past the end
      const i32x4q *p = Xv + (chunk0 + gl) * 512 + lane;
#pragma unroll
      for (int i = 0; i < 8; ++i) b[i] = __builtin_nontemporal_load(p + i * 64);
    };
#pragma unroll
    for (int p = 0; p < R - 1; ++p) load(xb[p], p);
    for (int t = 0; t < ntiles; t += TU) {
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int tt = t + u;
        const int tc = min(tt, ntiles - 1);
        const int64_t row0 = r_begin + (int64_t)tc * 64;
        // the tile's row metadata (lane: rows 16 rt + 4 g .. + 3 = {S, e} x 4 = 32 B per rt) and its
        // live / allow words, consumed by the epilogue
        f32x4 mr[4][2];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            mr[rt][h] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(rmeta + row0 + 16 * rt + 4 * g) + h);
        uint32_t lw, aw;
        bool w_ok;
        {
          const int64_t wi = (row0 >> 5) + (lane & 1);
          w_ok = wi < n_words;
          const int64_t wc = w_ok ? wi : n_words - 1;
          lw = __builtin_nontemporal_load(live + wc);
          aw = __builtin_nontemporal_load((allow ? allow : live) + wc);
        }
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          const int lc = u * KC + c;
          load(xb[(lc + R - 1) % R], tt * KC + c + R - 1);   // into the slot chunk lc - 1 used
          __builtin_amdgcn_sched_barrier(0);
          const int s = lc % R;
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
#pragma unroll
              for (int qt = 0; qt < QT; ++qt)
                acc[rt][qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xb[s][rt * 2 + kh], qf[c][kh][qt], acc[rt][qt], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (tt < ntiles) {   // ---- epilogue (wave-uniform condition)
          const uint32_t tw = w_ok ? (lw & aw) : 0u;
          const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)tw, 0);
          const uint32_t b1 = (uint32_t)__builtin_amdgcn_readlane((int)tw, 1);
          const bool full = (b0 & b1) == 0xffffffffu;
          const uint32_t live16 = full ? 0xffffu : lane_live16(((uint64_t)b1 << 32) | b0, g);
          const float S = mr[0][0][0];  // the lane's row group: one scale
          float E = 0.f;                // and the largest e_r of its rows
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int h = 0; h < 2; ++h) E = fmaxf(E, fmaxf(mr[rt][h][1], mr[rt][h][3]));
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) {
            int amax;
            if (full) {
              amax = acc[0][qt][0];
#pragma unroll
              for (int i = 1; i < 16; ++i) amax = max(amax, acc[i >> 2][qt][i & 3]);
            } else {                    // dead / filtered rows leave the maximum
              amax = INT32_MIN;
#pragma unroll
              for (int i = 0; i < 16; ++i) amax = max(amax, ((live16 >> i) & 1u) ? acc[i >> 2][qt][i & 3] : INT32_MIN);
            }
            const float A = sq[qt] * S, B = fmaf(-bq[qt], E, oaq[qt]);
            const float W = 2.0f * fmaf(bq[qt], E, aq[qt]) + 1e-6f;
            const bool pass = amax != INT32_MIN && fmaf(-A, (float)amax, B) <= sdq[qt];
            if (__ballot(pass) == 0) continue;   // wave-uniform: the common case
            uint32_t hm = 0;
            if (pass) {
#pragma unroll
              for (int i = 0; i < 16; ++i) hm |= (fmaf(-A, (float)acc[i >> 2][qt][i & 3], B) <= sdq[qt] ? 1u : 0u) << i;
              hm &= live16;
            }
            // slots: the query's running count + the hits of its lanes g' < g (lanes j, 16 + j, ...)
            const int c = __popc(hm);
            const int c0 = __shfl(c, j), c1 = __shfl(c, 16 + j), c2 = __shfl(c, 32 + j), c3 = __shfl(c, 48 + j);
            uint32_t slot = qcnt[qt] + (uint32_t)((g > 0 ? c0 : 0) + (g > 1 ? c1 : 0) + (g > 2 ? c2 : 0));
            qcnt[qt] += (uint32_t)(c0 + c1 + c2 + c3);
            if (hm) {
              const int64_t ob = ((int64_t)vg * kSQ + qt * 16 + j) * kQCap;
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                if ((hm >> i) & 1u) {
                  if (slot < (uint32_t)kQCap) {
                    const float lo = fmaf(-A, (float)acc[i >> 2][qt][i & 3], B);
                    const int64_t row = row0 + 16 * (i >> 2) + 4 * g + (i & 3);
                    out_keys[ob + slot] = ((uint64_t)f32_order(lo) << 32) | (uint64_t)(uint32_t)row;
                    out_up[ob + slot] = lo + W;
                  }
                  ++slot;
                }
              }
            }
          }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) acc[rt][qt] = i32x4q{0, 0, 0, 0};
      }
    }
  }
  if (g == 0) {
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) out_cnt[(int64_t)vg * kSQ + qt * 16 + j] = qcnt[qt];
  }
}

// Block-wide radix select over n values produced by val(i) (4 x 8-bit digits, re-reading them each
// pass): the kk-th smallest (0-based).
template <typename V>
__device__ inline uint32_t block_select_fn(V val, int n, int kk, uint32_t *hist) {
  __shared__ uint32_t s_prefix, s_rem;
  if (threadIdx.x == 0) {
    s_prefix = 0;
    s_rem = (uint32_t)kk;
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    const uint32_t prefix = s_prefix;
    const uint32_t hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t x = val(i);
      if ((x & hmask) == (prefix & hmask)) atomicAdd(&hist[(x >> shift) & 255u], 1u);
    }
    __syncthreads();
    // the digit: the bin b with C(b) <= rem < C(b + 1), C = the histogram's exclusive prefix sum --
    // wave 0, four bins per lane and a shuffle scan (was one thread walking the bins through
    // dependent LDS reads, up to 256 of them per digit)
    if (threadIdx.x < 64) {
      const int l = threadIdx.x;
      const uint32_t h0 = hist[4 * l], h1 = hist[4 * l + 1], h2 = hist[4 * l + 2], h3 = hist[4 * l + 3];
      const uint32_t sum = h0 + h1 + h2 + h3;
      uint32_t incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (l >= o) incl += v;
      }
      const uint32_t rem = s_rem, excl = incl - sum;
      if (excl <= rem && rem < incl) {   // exactly one lane (rem < the values left: kk < n)
        uint32_t r = rem - excl, b = 4u * l;
        if (r >= h0) {
          r -= h0;
          ++b;
          if (r >= h1) {
            r -= h1;
            ++b;
            if (r >= h2) {
              r -= h2;
              ++b;
            }
          }
        }
        s_prefix = prefix | (b << shift);
        s_rem = r;
      }
    }
    __syncthreads();
  }
  return s_prefix;
}

// K1q certification + exact re-rank, one kQRT-thread workgroup per query (see the file comment).
// 1. buffer offsets; 2. the candidates (lo key, up) gathered into LDS (kQGather of them; a larger
// set is read from the global buffers in place, L2-resident); 3. kth_up = the k-th smallest up;
// 4. band = candidates with lo <= kth_up (3': or the pilot bound); 5. exact fp64 distances, kQRows
// band rows per wave at a time with all their loads in flight (the arithmetic -- per-lane strided
// sums, xor-tree reduction -- is dense_rerank_kernel's, so K1q and K1c return bit-identical
// distances for a row); 6. top-k by rank.
//
// 3'. Pilot bound (without a full f16 plane, where the fp64 stage ranks the whole int8 band -- with
// the plane that stage re-scores the f16 band, ~k rows, and k pilot rows would double it to save f16
// reads alone; CM_K1Q_PILOT=0 -> pilot == 0 keeps kth_up alone, A/B).  kth_up ~ d_k + E, so the band
// lo <= kth_up is d~ <= d_k + 2E wide.  The candidates with up <= kth_up -- k of them plus ties on up
// -- are live, allowed rows; their exact distances are computed first (the fp64 stage's own function:
// the same bits), pkey = the k-th smallest of them (order key of the returned float), and the band is
// formed with bound = min(kth_up, pkey + kQPilotPad): d~ <= d_k + E, half the width.  The pilot rows
// are scored once: they stay out of the band (marked kQTaken where gathered) and their keys join the
// band's before the final ranking, so the fp64 stage never scores more rows than without the pilot.
// Safe: a row of the final top-k has a returned distance <= the k-th
// smallest returned distance of any k live, allowed rows, so <= pkey; its lo is a certified lower
// bound of the fp64 distance that value was rounded from, so lo <= pkey + the rounding; hence it is in
// the band.  The f16 stage and the wide re-rank need only an upper bound of the k-th distance that
// keeps every top-k row: the wide re-rank takes the tighter fb_bound unchanged.  More than kQSel
// rows with up <= kth_up (mass ties): no pilot.  The buffer-overflow exit leaves before it.
constexpr int kQGather = K1Q_RR;
constexpr int kQRows = 8;
constexpr int kQRerankLds = kQGather * 12;
// pkey's padding, in order-key steps (= float ulps).  E_r's 4e-6 slack covers the roundings between
// lo and the fp64 distance; the one it does not cover is that distance's rounding to the returned
// float, half an ulp of the result (the fp64 value is never a float denormal: 1 - cos is 0 or a
// multiple of 2^-53), so one step would do; four cost nothing in band size.
constexpr uint32_t kQPilotPad = 4;
constexpr int kQPilotRows = 2;   // pilot rows per wave and load round
constexpr uint64_t kQTaken = ~0ull;   // a gathered candidate the pilot scored (no key: its row would be 2^32 - 1)

// One wave's share of the exact fp64 stage: the rows src[c], c = c0 + r * stride < n (r < NR),
// all their loads in flight (past n: row n - 1 again, discarded); per-lane strided sums, xor-tree
// reduction (dense_rerank_kernel's arithmetic, so K1q and K1c return bit-identical distances for a
// row); lane 0 writes the key
// (f32_order(distance), row) to out[c].  out may be src (the pilot): entry c is read and written by
// one wave, in that order; the clamped read of entry n - 1 by another wave may see that entry's key
// instead of its row, and a key's low word -- all that is read -- is the row.
// M = ld / 64 strided elements per lane (12 at ld 768, 16 at ld 1024, 6 at ld 384), loaded unconditionally (rows
// are zero past dim, and so is s_q: the extra terms add exact zeros, so the sums equal
// dense_rerank_kernel's over dim).
template <int NR, int M, typename R>
__device__ __forceinline__ void q8_exact_rows(const R *src, int n, int c0, int stride, const float *__restrict__ C,
                                              int ld, const float *s_q, double qnrm, int lane, uint64_t *out) {
  float x[NR][M];
  uint32_t rows[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    rows[r] = (uint32_t)src[min(c0 + r * stride, n - 1)];
    const float *cr = C + (int64_t)rows[r] * ld + lane;
#pragma unroll
    for (int m = 0; m < M; ++m) x[r][m] = cr[64 * m];
  }
  double dq[NR], dc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    dq[r] = 0.0;
    dc[r] = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double xv = (double)x[r][m];
      dq[r] += xv * (double)s_q[lane + 64 * m];
      dc[r] += xv * xv;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      dq[r] += __shfl_xor(dq[r], o);
      dc[r] += __shfl_xor(dc[r], o);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (c0 + r * stride < n) {
        const float dist = (float)(1.0 - dq[r] / ((sqrt(dc[r]) + 1e-30) * (qnrm + 1e-30)));
        out[c0 + r * stride] = ((uint64_t)f32_order(dist) << 32) | rows[r];
      }
  }
}

// LD = the store's row stride: 768, or 1024 -- whose stores keep only the f16 plane's sample prefix
// (xh_rows_for), so that instance has no f16 stage, and ranks 6 rows per wave at a time in the fp64
// stage instead of 8: 6 x 16 = the 96 row registers of 8 x 12 (16 waves leave 128 VGPRs per lane).
// LD = 384 (dims 257-384) holds the whole f16 plane, for K1c / K1s, but has no f16 stage either
// (launch_coarse passes Xh = nullptr): the band goes straight to fp64 from the 1.5 KiB fp32 rows, 12
// rows per wave at a time, 12 x 6 = 72 row registers -- 16 x 6 = 96 spills 3 registers beside the 64 of
// the rows' fp64 sums (124 VGPRs at 12, 108 at 8, no scratch).
template <int LD>
__global__ void __launch_bounds__(kQRT) dense_rerank_q8_kernel(
    const uint64_t *__restrict__ keys, const float *__restrict__ ups, const uint32_t *__restrict__ cnts, int n_wg,
    int qs, int k, int nq, const float *__restrict__ C, int ld, int dim, const float *__restrict__ q,
    const float4 *__restrict__ qsc, const _Float16 *__restrict__ Xh, const _Float16 *__restrict__ Qh,
    const float *__restrict__ qnorm, const float *__restrict__ row_norms, float *__restrict__ out_dist,
    int64_t *__restrict__ out_row, int32_t *__restrict__ fb_mask, int32_t *__restrict__ fb_count,
    uint32_t *__restrict__ fb_bound, int pilot, unsigned long long *__restrict__ band_ctr) {
  const int qi = blockIdx.x;
  if (qi >= nq) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qp = qi / qs, ql = qi - qp * qs;   // qs: queries per pass of the buffer layout (K1q 256, K1q-s 32)
  static_assert(LD == 384 || LD == 768 || LD == 1024, "K1q re-rank: row strides with an int8 scan");
  // elements per lane; fp64-stage rows per wave
  constexpr int M = LD / 64, NR = LD == 768 ? kQRows : LD == 1024 ? 6 : 12;
  constexpr bool kF16Stage = LD == 768;
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  uint64_t *g_key = reinterpret_cast<uint64_t *>(dyn);                 // [kQGather]
  uint32_t *g_up = reinterpret_cast<uint32_t *>(dyn + kQGather * 8);   // [kQGather] f32_order(up)
  __shared__ uint32_t s_off[2049];
  __shared__ uint32_t hist[256];
  __shared__ float s_q[LD];
  __shared__ int s_flag, s_total, s_band;
  __shared__ uint64_t s_sel[kQSel];
  __shared__ int s_nsel;
  // the dynamic area's later lives: the int8 band's rows in g_up's space (dead after the kth_up
  // select), the f16 distances in g_key's first half and the f16 band's rows in its second (dead
  // after the band is formed), the fp64 keys over the f16 distances (dead after band2 is formed)
  static_assert(kQBand * 4 <= kQGather * 4 && kQBand * 4 <= kQGather * 4 && kQBand2 * 8 <= kQGather * 4, "K1q re-rank LDS");
  uint32_t *s_rows = g_up;                                                   // [kQBand]
  uint64_t *s_ex = g_key;                                                    // [kQBand2]
  if (tid == 0) {
    s_flag = 0;
    s_band = 0;
    s_nsel = 0;
  }
  __syncthreads();
  if (wave == 0) {  // buffer sizes -> offsets (n_wg <= 2048)
    uint32_t run = 0;
    for (int b0 = 0; b0 < n_wg; b0 += 64) {
      const int b = b0 + lane;
      uint32_t c = b < n_wg ? cnts[((int64_t)qp * n_wg + b) * qs + ql] : 0u;
      if (c > (uint32_t)kQCap) {
        s_flag = 1;
        c = kQCap;
      }
      uint32_t incl = c;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      if (b < n_wg) s_off[b] = run + incl - c;
      run += __shfl(incl, 63);
    }
    if (lane == 0) {
      s_off[n_wg] = run;
      s_total = (int)run;
    }
  }
  __syncthreads();
  const int total = s_total;
  auto slot_of = [&](int jj) -> int64_t {  // candidate jj: its buffer = the last b with s_off[b] <= jj
    int lo = 0, hi = n_wg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_off[mid] <= (uint32_t)jj) lo = mid;
      else hi = mid - 1;
    }
    return (((int64_t)qp * n_wg + lo) * qs + ql) * kQCap + (jj - s_off[lo]);
  };
  const bool gathered = total <= kQGather;
  if (gathered) {
#pragma unroll 4
    for (int jj = tid; jj < total; jj += kQRT) {
      const int64_t sl = slot_of(jj);
      g_key[jj] = keys[sl];
      g_up[jj] = f32_order(ups[sl]);
    }
  }
  for (int i = tid; i < LD; i += kQRT) s_q[i] = i < dim ? q[(int64_t)qi * dim + i] : 0.f;  // zero past dim
  __syncthreads();
  auto key_at = [&](int jj) -> uint64_t { return gathered ? g_key[jj] : keys[slot_of(jj)]; };
  auto up_at = [&](int jj) -> uint32_t { return gathered ? g_up[jj] : f32_order(ups[slot_of(jj)]); };
  // kth_up: the k-th smallest d~ + E_r (fewer than k candidates: all of them form the band)
  uint32_t tkey = 0xffffffffu;
  if (total >= k) tkey = block_select_fn(up_at, total, k - 1, hist);
  if (s_flag) {   // a (group, query) buffer overflowed: the candidate set is incomplete, but kth_up over
                  // the kept candidates still bounds the k-th distance -> the wide re-rank re-scans those groups
    if (tid == 0) {
      fb_mask[qi] = 2;
      fb_bound[qi] = tkey;
      atomicAdd(fb_count, 1);
    }
    return;
  }
  const double qnrm = (double)qsc[qi].w;
  // 3'. pilot bound (see above): s_sel / s_nsel are free until the final ranking
  uint32_t bound = tkey;
  int npilot = 0;
  if (pilot && Xh == nullptr && total >= k) {
    for (int jj = tid; jj < total; jj += kQRT) {
      if (up_at(jj) <= tkey) {
        const int p = atomicAdd(&s_nsel, 1);
        if (p < kQSel) s_sel[p] = (uint64_t)jj;
      }
    }
    __syncthreads();
    npilot = s_nsel;             // >= k
    __syncthreads();
    if (tid == 0) s_nsel = 0;    // as the final ranking expects it (barriers in between)
    if (npilot <= kQSel) {
      static_assert(kQSel <= kQRT, "one thread per pilot row");
      if (tid < npilot) {
        const int jj = (int)s_sel[tid];
        s_sel[tid] = (uint32_t)key_at(jj);    // the row; its exact key below
        if (gathered) g_key[jj] = kQTaken;    // scored here: not a band row (a candidate left in the
      }                                       // global buffers is told by its up)
      __syncthreads();
      // row c on wave c % kQRW: k + ties <= kQRW * kQPilotRows = 32 rows are one round of loads
      for (int c0 = wave; c0 < npilot; c0 += kQRW * kQPilotRows)
        q8_exact_rows<kQPilotRows, M>(s_sel, npilot, c0, kQRW, C, ld, s_q, qnrm, lane, s_sel);
      __syncthreads();
      const uint32_t pkey = block_select_fn([&](int i) { return (uint32_t)(s_sel[i] >> 32); }, npilot, k - 1, hist);
      bound = min(tkey, pkey <= 0xffffffffu - kQPilotPad ? pkey + kQPilotPad : 0xffffffffu);
    } else {
      npilot = 0;
    }
  }
  const bool pilot_by_up = npilot > 0 && !gathered;
  for (int jj = tid; jj < total; jj += kQRT) {
    const uint64_t key = key_at(jj);
    if (key == kQTaken || (pilot_by_up && up_at(jj) <= tkey)) continue;   // a pilot row
    if (bound == 0xffffffffu || (uint32_t)(key >> 32) <= bound) {   // lo <= bound (order-preserving keys)
      const int p = atomicAdd(&s_band, 1);
      if (p < kQBand) s_rows[p] = (uint32_t)key;
    }
  }
  __syncthreads();
  const int band = s_band;
  if (band + npilot > kQBand) {   // complete candidate set, band too wide for LDS: the wide re-rank (fb_mask 2)
    if (tid == 0) {
      fb_mask[qi] = 2;
      fb_bound[qi] = bound;
      atomicAdd(fb_count, 1);
      if (npilot) atomicAdd(band_ctr, (unsigned long long)npilot);
    }
    return;
  }
  if (tid == 0) {
    fb_mask[qi] = 0;
    fb_bound[qi] = 0u;   // not sent to the wide re-rank (no kth_up key is 0): its slot ranking counts the others
  }
  const uint32_t *band_rows = s_rows;   // the rows the fp64 stage re-ranks: the f16 band, or (no full
  int band2 = band;                     // f16 plane, xh_rows_for) the whole int8 band
  if (kF16Stage && Xh != nullptr) {
  // 5'. f16 middle stage (K1c's certificate): the band rows' coarse distances from the f16 plane,
  // d_h = 1 - xh . qh (fp32), |(1 - xn . qn) - d_h| <= Eh (coarse_err); kth_h = the k-th smallest
  // d_h + Eh over the band (>= the true k-th distance: the band holds every true top-k row), band2 =
  // the rows with d_h - Eh <= kth_h -- it still holds every true top-k row, and it is the size of
  // K1c's band (~30 rows) instead of the int8 band's ~1000: the fp64 stage reads 1.5 KiB per band
  // row here instead of 3 KiB, and 3 KiB only per band2 row.  Half a wave per row: lane l of the
  // half reads the row's 16-B plane pieces l, l + 32, l + 64 (piece p = k 64 (p >> 3) + 32 ((p >> 2)
  // & 1) + 8 (p & 3) .. + 7), v_dot2_f32_f16 products, a 32-lane xor tree.
  float *s_dh = reinterpret_cast<float *>(dyn);                             // [kQBand]
  uint32_t *s_rows2 = reinterpret_cast<uint32_t *>(dyn + kQGather * 4);     // [kQBand]
  const float Eh = coarse_err(qnorm, qi, row_norms, dim);
  {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const int hl = lane & 31, hh = lane >> 5;
    f16x8 qv[3];
    int kof[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int pc = hl + 32 * u;
      kof[u] = 64 * (pc >> 3) + 32 * ((pc >> 2) & 1) + 8 * (pc & 3);
      qv[u] = *reinterpret_cast<const f16x8 *>(Qh + (int64_t)qi * ld + kof[u]);
    }
    constexpr int RP = 4;   // row pairs per wave and iteration (12 loads per lane in flight)
    for (int c0 = wave * 2 * RP; c0 < band; c0 += kQRW * 2 * RP) {
      f16x8 xv[RP][3];
#pragma unroll
      for (int rp = 0; rp < RP; ++rp) {
        const int c = min(c0 + 2 * rp + hh, band - 1);
        const int64_t row = s_rows[c];
        const int64_t tile = row >> 6;
        const int rr = (int)(row & 63), rt = rr >> 4, jj = rr & 15;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int pc = hl + 32 * u, cch = pc >> 3, sb = (pc >> 2) & 1, gg = pc & 3;
          xv[rp][u] = *reinterpret_cast<const f16x8 *>(   // (row, k-half) runs of 64 B (plane_off)
              Xh + ((((tile * (ld >> 6) + cch) * 8 + rt * 2 + sb) << 9) + ((jj * 4 + gg) << 3)));
        }
      }
#pragma unroll
      for (int rp = 0; rp < RP; ++rp) {
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int e = 0; e < 8; e += 2)
            acc = __builtin_amdgcn_fdot2(h2{xv[rp][u][e], xv[rp][u][e + 1]}, h2{qv[u][e], qv[u][e + 1]}, acc, false);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        const int c = c0 + 2 * rp + hh;
        if (hl == 0 && c < band) s_dh[c] = 1.0f - acc;
      }
    }
  }
  __syncthreads();
  {
    const uint32_t kth_h = band >= k ? block_select_fn([&](int i) { return f32_order(s_dh[i] + Eh); }, band, k - 1, hist)
                                     : 0xffffffffu;
    if (tid == 0) s_band = 0;
    __syncthreads();
    for (int c = tid; c < band; c += kQRT)
      if (kth_h == 0xffffffffu || f32_order(s_dh[c] - Eh) <= kth_h) s_rows2[atomicAdd(&s_band, 1)] = s_rows[c];
    __syncthreads();
  }
  band2 = s_band;
  band_rows = s_rows2;
  if (band2 > kQBand2) {   // (the f16 band holds the int8 band's near-ties: the wide re-rank)
    if (tid == 0) {
      fb_mask[qi] = 2;
      fb_bound[qi] = bound;
      atomicAdd(fb_count, 1);
    }
    return;
  }
  }   // Xh != nullptr (without it: s_ex = g_key's 64 KiB holds kQBand keys beside s_rows in g_up's space)
  if (tid == 0) atomicAdd(band_ctr, (unsigned long long)(band2 + npilot));
  for (int c0 = wave * NR; c0 < band2; c0 += kQRW * NR)
    q8_exact_rows<NR, M>(band_rows, band2, c0, 1, C, ld, s_q, qnrm, lane, s_ex);
  if (tid < npilot) s_ex[band2 + tid] = s_sel[tid];   // the pilot rows' keys join the band's
  band2 += npilot;
  __syncthreads();
  // top-k of the band: the k-th smallest distance (radix select over the keys' high words), then the
  // rows at or below it (k plus exact distance ties: a handful) ranked by their full keys
  const uint32_t thi = band2 > k ? block_select_fn([&](int i) { return (uint32_t)(s_ex[i] >> 32); }, band2, k - 1, hist)
                                : 0xffffffffu;
  for (int c = tid; c < band2; c += kQRT) {
    const uint64_t key = s_ex[c];
    if ((uint32_t)(key >> 32) <= thi) {
      const int p = atomicAdd(&s_nsel, 1);
      if (p < kQSel) s_sel[p] = key;
    }
  }
  __syncthreads();
  const int nsel = s_nsel;
  const uint64_t *cand = nsel <= kQSel ? s_sel : s_ex;  // more ties than kQSel: rank over the whole band
  const int ncand = nsel <= kQSel ? nsel : band2;
  for (int c = tid; c < ncand; c += kQRT) {
    const uint64_t key = cand[c];
    int rank = 0;
    for (int i = 0; i < ncand; ++i) rank += cand[i] < key ? 1 : 0;
    if (rank < k) {
      out_dist[(int64_t)qi * k + rank] = f32_unorder((uint32_t)(key >> 32));
      out_row[(int64_t)qi * k + rank] = (int64_t)(uint32_t)key;
    }
  }
  for (int i = band2 + tid; i < k; i += kQRT) {
    out_dist[(int64_t)qi * k + i] = 0.f;
    out_row[(int64_t)qi * k + i] = -1;
  }
}

// K1q's wide re-rank (round 5): a query whose int8 band (> kQBand rows) or f16 band (> kQBand2) does not
// fit the re-rank's LDS -- near-duplicate clusters: every row within the bounds' width of the k-th
// distance is a band row -- but whose candidate buffers did not overflow (the candidate set holds every
// row with lo <= seed, hence every true top-k row) is finished here instead of by the exact fp32 scan
// of all rows: every candidate with lo <= kth_up (fb_bound) gets its exact fp64 distance from the fp32
// row (the same per-lane arithmetic as dense_rerank_q8_kernel, so the same bits), into a global slot
// of kWideCap keys; then the k-th smallest distance (radix select), the <= kQSel rows at or below it
// ranked by full key.  One 1024-thread workgroup per failing query, at most kWideSlots queries per
// search (the first by query index); beyond that, a band over kWideCap rows or more than kQSel exact ties, the query keeps
// fb_mask 1 for the exact pass.  Gated: every workgroup leaves at once when no query failed.
constexpr int kWideSlots = 16;
constexpr int kWideCap = 1 << 16;
constexpr int kWideThreads = 1024;
constexpr int kWideOvf = 64;    // overflowed (group, query) buffers one query may re-scan
template <int LD>
__global__ void __launch_bounds__(kWideThreads) dense_rerank_wide_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ cnts, int n_wg, int qs, int k, int nq,
    const float *__restrict__ C, int ld, int dim, const float *__restrict__ q, const float4 *__restrict__ qsc,
    const float *__restrict__ qbase,
    const _Float16 *__restrict__ Xh, const _Float16 *__restrict__ Qh, const float *__restrict__ qnorm,
    const float *__restrict__ row_norms, const int8_t *__restrict__ Xq, const float2 *__restrict__ rmeta,
    const int8_t *__restrict__ Qq, const uint32_t *__restrict__ live, const uint32_t *__restrict__ allow,
    int64_t n_words, int64_t rows_per_wg, int64_t rows_end,
    float *__restrict__ out_dist, int64_t *__restrict__ out_row, int32_t *__restrict__ fb_mask,
    int32_t *__restrict__ fb_count, const uint32_t *__restrict__ fb_bound, int32_t *__restrict__ wide_ctr,
    uint32_t *__restrict__ wide_rows, uint64_t *__restrict__ wide_keys) {
  const int qi = blockIdx.x;
  if (qi >= nq || *fb_count == 0 || fb_mask[qi] != 2) return;   // uniform per workgroup
  static_assert(LD == 384 || LD == 768 || LD == 1024, "K1q wide re-rank: row strides with an int8 scan");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = kWideThreads / 64;
  const int qp = qi / qs, ql = qi - qp * qs;
  __shared__ uint32_t s_off[2049];
  __shared__ uint32_t hist[256];
  __shared__ float s_q[LD];
  __shared__ uint64_t s_sel[kQSel];
  __shared__ int s_ovf[kWideOvf];
  __shared__ int s_slot, s_n, s_nsel, s_total, s_novf;
  if (tid == 0) {
    s_slot = 0;
    s_n = 0;
    s_nsel = 0;
    s_novf = 0;
  }
  __syncthreads();
  // slot = this query's rank among the queries the re-rank sent here (fb_bound != 0; written by the
  // re-rank for every query, only read here): the first kWideSlots of them by query index get a slot,
  // whatever order the workgroups run in -- an allocator handed them out in arrival order, so with more
  // than kWideSlots failing queries the same search returned fp64 or fp32-pass distance bits by chance
  {
    int before = 0;
    for (int j = tid; j < qi; j += kWideThreads) before += fb_bound[j] != 0u ? 1 : 0;
    if (before) atomicAdd(&s_slot, before);
  }
  if (wave == 0) {  // buffer sizes -> offsets; an overflowed buffer's group is re-scanned below instead
    uint32_t run = 0;
    for (int b0 = 0; b0 < n_wg; b0 += 64) {
      const int b = b0 + lane;
      uint32_t c = b < n_wg ? cnts[((int64_t)qp * n_wg + b) * qs + ql] : 0u;
      if (c > (uint32_t)kQCap) {
        const int o = atomicAdd(&s_novf, 1);
        if (o < kWideOvf) s_ovf[o] = b;
        c = 0;
      }
      uint32_t incl = c;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      if (b < n_wg) s_off[b] = run + incl - c;
      run += __shfl(incl, 63);
    }
    if (lane == 0) {
      s_off[n_wg] = run;
      s_total = (int)run;
    }
  }
  for (int i = tid; i < LD; i += kWideThreads) s_q[i] = i < dim ? q[(int64_t)qi * dim + i] : 0.f;  // zero past dim
  __syncthreads();
  const int slot = s_slot;
  const int novf = s_novf;
  if (slot >= kWideSlots || novf > kWideOvf) {   // more failing queries than slots / too many overflowed
    if (tid == 0) fb_mask[qi] = 1;                // groups: this one takes the exact pass
    return;
  }
  uint32_t *rows = wide_rows + (int64_t)slot * kWideCap;
  uint64_t *wk = wide_keys + (int64_t)slot * kWideCap;
  const uint32_t tkey = fb_bound[qi];
  const int total = s_total;
  for (int jj = tid; jj < total; jj += kWideThreads) {   // band: lo <= kth_up
    int lo = 0, hi = n_wg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_off[mid] <= (uint32_t)jj) lo = mid;
      else hi = mid - 1;
    }
    const uint64_t key = keys[(((int64_t)qp * n_wg + lo) * qs + ql) * kQCap + (jj - s_off[lo])];
    if ((uint32_t)(key >> 32) <= tkey) {
      const int p = atomicAdd(&s_n, 1);
      if (p < kWideCap) rows[p] = (uint32_t)key;
    }
  }
  // no full f16 plane (xh_rows_for): the overflowed groups' live & allowed rows are filtered on the
  // int8 plane with the scan's own per-row bound, lo_r = base_q - a_q - b_q e_r - s_q S_r acc_r <= kth_up
  // (acc_r exact in int32); one wave per row, lane l < LD / 16 (24, 48, or all 64) its 16-B piece
  // (chunk l / 8, k-half (l / 4) % 2, lane group l % 4) of the row and of the query fragment, sdot4
  // products, a 64-lane xor tree
  if (novf > 0 && Xh == nullptr) {
    const float4 qs4 = qsc[qi];
    const float qb = qbase[qi];   // base_q
    const int64_t qt = qi >> 4;
    const int jq = qi & 15;
    const int c = lane >> 3, kh = (lane >> 2) & 1, gq = lane & 3;
    i32x4q qv = {0, 0, 0, 0};
    if (lane < LD / 16)
      qv = *reinterpret_cast<const i32x4q *>(Qq + ((((qt * (ld >> 7) + c) * 2 + kh) << 10) + ((gq * 16 + jq) << 4)));
    for (int g = 0; g < novf; ++g) {
      const int64_t r0 = (int64_t)s_ovf[g] * rows_per_wg, r1 = min(r0 + rows_per_wg, rows_end);
      for (int64_t row = r0 + wave; row < r1; row += NW) {   // uniform per wave
        if ((row >> 5) >= n_words) break;
        const uint32_t lw = live[row >> 5] & (allow ? allow[row >> 5] : 0xffffffffu);
        if (!((lw >> (row & 31)) & 1u)) continue;
        const int64_t tile = row >> 6;
        const int rr = (int)(row & 63), rt = rr >> 4, jj = rr & 15;
        int acc = 0;
        if (lane < LD / 16) {
          const i32x4q xv = *reinterpret_cast<const i32x4q *>(
              Xq + ((((tile * (ld >> 7) + c) * 8 + rt * 2 + kh) << 10) + ((gq * 16 + jj) << 4)));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_sdot4(xv[e], qv[e], acc, false);
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        const float2 m = rmeta[row];
        const float lo = fmaf(-(qs4.x * m.x), (float)acc, fmaf(-qs4.z, m.y, qb - qs4.y));
        if (lane == 0 && f32_order(lo) <= tkey) {
          const int p = atomicAdd(&s_n, 1);
          if (p < kWideCap) rows[p] = (uint32_t)row;
        }
      }
    }
  }
  // the overflowed groups' live & allowed rows, filtered on the f16 plane: d_h - Eh <= kth_up (the f16
  // stage of dense_rerank_q8_kernel: half a wave per row, its 16-B plane pieces l, l + 32, l + 64)
  if (LD == 768 && novf > 0 && Xh != nullptr) {   // (an ld 1024 store never holds the full plane)
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const float Eh = coarse_err(qnorm, qi, row_norms, dim);
    const int hl = lane & 31, hh = lane >> 5;
    f16x8 qv[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int pc = hl + 32 * u;
      qv[u] = *reinterpret_cast<const f16x8 *>(Qh + (int64_t)qi * ld + 64 * (pc >> 3) + 32 * ((pc >> 2) & 1) + 8 * (pc & 3));
    }
    for (int g = 0; g < novf; ++g) {
      const int64_t r0 = (int64_t)s_ovf[g] * rows_per_wg, r1 = min(r0 + rows_per_wg, rows_end);
      for (int64_t row = r0 + 2 * wave + hh; row < r1; row += 2 * NW) {   // uniform per half-wave
        if ((row >> 5) >= n_words) break;   // past the store's last word (live and allow hold ceil(size / 32))
        const uint32_t lw = live[row >> 5] & (allow ? allow[row >> 5] : 0xffffffffu);
        if (!((lw >> (row & 31)) & 1u)) continue;
        const int64_t tile = row >> 6;
        const int rr = (int)(row & 63), rt = rr >> 4, jj = rr & 15;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int pc = hl + 32 * u, cch = pc >> 3, sb = (pc >> 2) & 1, gg = pc & 3;
          const f16x8 xv = *reinterpret_cast<const f16x8 *>(
              Xh + ((((tile * (ld >> 6) + cch) * 8 + rt * 2 + sb) << 9) + ((jj * 4 + gg) << 3)));
#pragma unroll
          for (int e = 0; e < 8; e += 2)
            acc = __builtin_amdgcn_fdot2(h2{xv[e], xv[e + 1]}, h2{qv[u][e], qv[u][e + 1]}, acc, false);
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 32);
        if (hl == 0 && f32_order(1.0f - acc - Eh) <= tkey) {
          const int p = atomicAdd(&s_n, 1);
          if (p < kWideCap) rows[p] = (uint32_t)row;
        }
      }
    }
  }
  __syncthreads();
  const int n = s_n;
  if (n > kWideCap) {
    if (tid == 0) fb_mask[qi] = 1;
    return;
  }
  // exact fp64 distances, dense_rerank_q8_kernel's arithmetic (LD / 64 strided elements per lane)
  const double qnrm = (double)qsc[qi].w;
  constexpr int M = LD / 64, WR = 4;   // rows per wave and iteration (<= 128 VGPRs at 16 waves)
  for (int c0 = wave * WR; c0 < n; c0 += NW * WR) {
    float x[WR][M];
    uint32_t rr[WR];
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      const int c = min(c0 + r, n - 1);
      rr[r] = rows[c];
      const float *cr = C + (int64_t)rr[r] * ld + lane;
#pragma unroll
      for (int m = 0; m < M; ++m) x[r][m] = cr[64 * m];
    }
    double dq[WR], dc[WR];
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      dq[r] = 0.0;
      dc[r] = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double xv = (double)x[r][m];
        dq[r] += xv * (double)s_q[lane + 64 * m];
        dc[r] += xv * xv;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int r = 0; r < WR; ++r) {
        dq[r] += __shfl_xor(dq[r], o);
        dc[r] += __shfl_xor(dc[r], o);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < WR; ++r)
        if (c0 + r < n) {
          const float dist = (float)(1.0 - dq[r] / ((sqrt(dc[r]) + 1e-30) * (qnrm + 1e-30)));
          wk[c0 + r] = ((uint64_t)f32_order(dist) << 32) | rr[r];
        }
    }
  }
  __threadfence_block();
  __syncthreads();
  const uint32_t thi = n > k ? block_select_fn([&](int i) { return (uint32_t)(wk[i] >> 32); }, n, k - 1, hist)
                             : 0xffffffffu;
  for (int c = tid; c < n; c += kWideThreads) {
    const uint64_t key = wk[c];
    if ((uint32_t)(key >> 32) <= thi) {
      const int p = atomicAdd(&s_nsel, 1);
      if (p < kQSel) s_sel[p] = key;
    }
  }
  __syncthreads();
  const int nsel = s_nsel;
  if (nsel > kQSel) {   // more exact ties than the ranking buffer: the exact pass
    if (tid == 0) fb_mask[qi] = 1;
    return;
  }
  for (int c = tid; c < nsel; c += kWideThreads) {
    const uint64_t key = s_sel[c];
    int rank = 0;
    for (int i = 0; i < nsel; ++i) rank += s_sel[i] < key ? 1 : 0;
    if (rank < k) {
      out_dist[(int64_t)qi * k + rank] = f32_unorder((uint32_t)(key >> 32));
      out_row[(int64_t)qi * k + rank] = (int64_t)(uint32_t)key;
    }
  }
  for (int i = n + tid; i < k; i += kWideThreads) {
    out_dist[(int64_t)qi * k + i] = 0.f;
    out_row[(int64_t)qi * k + i] = -1;
  }
  if (tid == 0) {
    fb_mask[qi] = 0;
    atomicSub(fb_count, 1);
    atomicAdd(wide_ctr + 1, 1);   // [1]: queries finished here ([0], once the slot allocator, is unused)
  }
}
