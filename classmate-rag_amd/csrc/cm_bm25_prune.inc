// Pruned BM25 search (K2a tail pass + bound + K2 re-score) — included by
// cm_bm25.hip inside namespace cm, after the K2 range kernel and its helpers.
//
// Exactness argument (DESIGN.md §4 "K2a"): every query term is either a head
// term (dense tf tile) or a tail term (CSR postings); a query without tail terms
// walks the postings of its rarest head term instead (bm25_qcand_kernel).  A
// document holding such a candidate-generating term is a *tail candidate*; K2a scores every tail candidate exactly
// (same fp64 formula and term order as K2).  A document with head terms only
// scores at most UB(q, r) = sum over the query's head terms (duplicates
// included) of max(idf, 0) * ratio(maxtf(h, r), mindl(r)), where maxtf is the
// largest tf byte of head h in range r and mindl the shortest document of the
// range (the ratio tf*2.5/(tf+K_d) grows with tf and shrinks with dl).  With
// T = the k-th best tail-candidate score (a lower bound of the true k-th best),
// ranges where UB*(1+1e-9) < T cannot hold a head-only document of the top-k
// (strictly below, so row tie-breaks do not matter), and neither can a document
// with no query term (score 0 <= UB).  Every other (query, range) pair — and
// every range of a query with no positive T, more than 16 terms, or a range
// whose tail lists overflow LDS — is re-scored in full by K2, whose complete
// range list replaces the tail pass's.

// K2a's LDS list capacity and occupancy target: 320 slots (6.25 KB per wave) with 5 waves per
// SIMD measured 2.26 vs 2.39 ms for 512 slots at 4 (10M docs, B = 256; bit-identical results);
// 256 slots overflow often enough that the K2 re-score costs more than the occupancy gains
#ifndef K2A_CAP
#define K2A_CAP 320
#endif
// ranges per K2a iteration: a "super-range" of K2A_SUB consecutive 1024-doc ranges is gathered,
// scored and ranked in one pass (its postings are one contiguous segment per term), amortising
// the per-iteration prefix / gather / rank / synchronisation over ~SUB x more candidates; the
// output is unchanged -- one k-slot list per (query, range), candidates grouped by query and range
#ifndef K2A_SUB
#define K2A_SUB 4
#endif
// planned blocks whose loads K2b issues together (2: 3.89 -> 3.73 ms BM25 search; 4 and 6 were
// slower than 1 -- wasted loads of half-filled groups, not latency, dominate beyond 2)
#ifndef K2B_U
#define K2B_U 2
#endif
#ifndef K2A_WPE
#define K2A_WPE 5
#endif
// Waves per K2a block.  The waves never synchronise, but a block gives its LDS back (and lets the
// next block in) only when its slowest wave ends, and a wave's work is Zipf-skewed (p50 18 us, p99
// 72 us): 4-wave blocks held 2.6 of the 5 waves per SIMD the kernel is built for, evenly over the
// whole launch, one-wave blocks hold 3.8 (profiles/k2a_tail.txt).  10M docs, B = 256, alone, same
// box: 1.128 ms at 4, 0.872 at 2, 0.844 at 1 (profiles/k2a_order_ab.txt; bit-identical results).
#ifndef K2A_W
#define K2A_W 1
#endif
// K2a's candidate scoring has one path: packed head tf gathers and the length load issued up
// front, tail tf from the LDS lists, the fp32 bound against T, the fp64 score.  Variants that were
// built, measured slower and removed (the commit before their removal is the last that builds them):
//  * a gather-free pre-bound before the gathers, from per-(head, 64-doc block) bytes (2.06 vs 1.38
//    ms, profiles/r05_k2a_prebound_ab.txt), from range-level bounds in LDS and from 16-doc
//    sub-block bytes (1.75 vs 1.13 ms): DESIGN.md §6 "Measured and not adopted" and §9 item 4,
//    profiles/r05_bm25_tseed_ab.txt, profiles/r06_seed_sample_k2a_prebound_ab.txt;
//  * the length gather behind a bound at the block's shortest length (same §6 paragraph and
//    r05 profile), and a branch-free fp32 sum (profiles/r06_k2b_uniform_ab.txt);
//  * one register per term tf instead of two per register (profiles/r04c_k2a_pack_ab.txt).
// Every bound placed before the gathers serialises their latency; the others cost spilled VGPRs.

// diagnostic variant builds only (off in the product; no output depends on it): every K2a wave
// records {XCC << 32 | unit + 1, start, end (s_memrealtime ticks, 100 MHz), tail postings loaded} for
// each work unit it runs, read back by cm_bm25_k2a_trace (tools/bm25_probe.py --k2a-trace)
#ifndef K2A_TRACE
#define K2A_TRACE 0
#endif
#if K2A_TRACE
__device__ uint64_t *g_k2a_trace;
#endif
typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));
constexpr int kCandCap = K2A_CAP;  // tail postings per (wave, range) in K2a; more -> K2 re-scores the range

__device__ inline int lds_find(const int32_t *a, int n, int32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && a[lo] == x) ? lo : -1;
}

// fp32 score bounds (planner, K2a/K2b candidate pre-check): inflated by kPlanSlack >> the
// < 1e-6 relative rounding of <= 16 fp32 terms, so a bound below T proves the exact score is.
constexpr float kPlanSlack = 1.0f + 2e-5f;
// idf rounded up to fp32 (a positive idf stays positive and normal; <= 0 -> 0: a term with
// idf <= 0 adds idf * ratio <= 0, so an upper bound may leave it out)
__device__ inline float idf_up(double x) { return x > 0.0 ? fmaxf(__double2float_ru(x), 1.2e-38f) : 0.0f; }
// K_d lower bound in fp32: 1.5 (0.25 + 0.75 dl / avgdl) with 1 / avgdl rounded down
__device__ inline float inv_avg_lo(double avgdl) { return (float)(1.0 / avgdl) * (1.0f - 1e-6f); }
__device__ inline float kd_lo32(int32_t dlen, float inv_avg) { return 1.5f * (0.25f + 0.75f * (float)dlen * inv_avg); }
// upper bound of one term's tf.2.5 / (tf + K_d) (the slack absorbs the approximate reciprocal)
__device__ inline float ratio_up32(uint32_t tf, float kd) {
  const float t = (float)tf;
  return (t * 2.5f) * __builtin_amdgcn_rcpf(t + kd);
}
template <typename TF>
__global__ void __launch_bounds__(64 * K2A_W) __attribute__((amdgpu_waves_per_eu(K2A_WPE)))
    bm25_tail_kernel(int nq, const int64_t *__restrict__ bounds, int nr, int rpw,
                     const int32_t *__restrict__ post_doc, const TF *__restrict__ post_tf,
                     const uint8_t *__restrict__ headtf, int64_t npad,
                     const int32_t *__restrict__ dl, const uint32_t *__restrict__ live,
                     const uint32_t *__restrict__ allow, const double *__restrict__ avgdl_p, int k,
                     uint64_t *__restrict__ cand_key, uint32_t *__restrict__ cand_row,
                     unsigned long long *__restrict__ thr_key, uint8_t *__restrict__ need,
                     const int32_t *__restrict__ qd_code, const int32_t *__restrict__ qd_term,
                     const double *__restrict__ qd_idf, const int32_t *__restrict__ qd_tb,
                     const int32_t *__restrict__ qd_len, int dbg) {
  constexpr int W = K2A_W;
  const double avgdl = *avgdl_p;
#ifndef CM_ABLATION
  dbg = 0;  // product build: the ablation branches fold away
#endif
  __shared__ int32_t s_pdoc[W][kCandCap];
  __shared__ uint16_t s_ptf[W][kCandCap];
  __shared__ uint64_t s_key[W][kCandCap];
  __shared__ uint8_t s_eln[W][kCandCap];
  __shared__ int32_t s_t[W][64], s_h[W][64], s_off[W][64], s_cnt[W][64];
  __shared__ double s_idf[W][64];
  __shared__ float s_fi[W][64];  // idf rounded up to fp32 (0 when <= 0) for the candidates' bound
  __shared__ double s_tq[W][kQPerWave];  // per query of the wave: T of this iteration (score)
  const float inv_avg = inv_avg_lo(avgdl);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // same XCD-aware wave -> (query group, run of ranges) mapping as K2
  const int nb = gridDim.x;
  const int b = blockIdx.x;
  const int per = nb >> 3, rem = nb & 7, x = b & 7, y = b >> 3;
  const int lb = (x < rem ? x * (per + 1) : rem * (per + 1) + (x - rem) * per) + y;
  const int nqg = (nq + kQPerWave - 1) / kQPerWave;
  const int wid = lb * W + wave;
  const int qg = wid % nqg;
  const int q0 = qg * kQPerWave;
  const int rg = wid / nqg;
  const int r0 = rg * rpw, r1 = min(r0 + rpw, nr);
  if (r0 >= r1) return;  // whole wave
#if K2A_TRACE
  const uint64_t tr_t0 = __builtin_amdgcn_s_memrealtime();
  uint64_t tr_post = 0;
#endif
  const int nqw = min(kQPerWave, nq - q0);
  int32_t *pdoc = s_pdoc[wave];
  uint16_t *ptf = s_ptf[wave];
  uint64_t *skey = s_key[wave];
  uint8_t *eln = s_eln[wave];
  int32_t *st = s_t[wave], *sh = s_h[wave], *soff = s_off[wave], *scnt = s_cnt[wave];
  double *sidf = s_idf[wave];
  const int64_t bstride = nr + 1;
  // ---- term descriptors (lane 16q + j <-> term j of query q0 + q); queries with more
  // than kTermLanes terms are left to the re-score pass
  const int my_q = lane / kTermLanes, my_j = lane % kTermLanes;
  // (the per-query descriptors of bm25_qcand_kernel: one load level, slots past the query's
  // length hold term -1, code 0, idf 0)
  int my_tb = 0, my_L = 0, my_c = 0;
  int32_t my_t = -1;
  double my_idf = 0.0;
  if (my_q < nqw) {
    const int64_t di = (int64_t)(q0 + my_q) * kTermLanes + my_j;
    my_tb = qd_tb[q0 + my_q];
    my_L = qd_len[q0 + my_q];
    my_t = qd_term[di];
    my_c = qd_code[di];
    my_idf = qd_idf[di];
  }
  const bool q_ok = my_q < nqw && my_L <= kTermLanes;
  // bits 0..3 <- ballot bits of lanes 0, 16, 32, 48
  const uint64_t okb = __ballot(q_ok && my_j == 0);
  const uint32_t qokm = (uint32_t)((okb & 1u) | ((okb >> 15) & 2u) | ((okb >> 30) & 4u) | ((okb >> 45) & 8u));
  const bool has_term = q_ok && my_j < my_L;
  const int my_i = my_tb + my_j;
  if (!has_term) {
    my_t = -1;
    my_c = 0;
    my_idf = 0.0;
  }
  const int32_t my_h = (my_c & 0x3fffffff) - 1;
  const bool tail = my_t >= 0 && ((my_c >> 30) & 1);  // candidate generator: tail term or designated head
  st[lane] = my_t;
  sh[lane] = my_h;
  sidf[lane] = my_idf;
  s_fi[wave][lane] = idf_up(my_idf);
  constexpr int SUB = K2A_SUB;
  constexpr int NG = kQPerWave * SUB;  // (query, range) groups of one iteration: g = q * SUB + sub
  int64_t my_lo = 0, my_hi = 0;
  if (tail) {
    my_lo = bounds[(int64_t)my_i * bstride + r0];
    my_hi = bounds[(int64_t)my_i * bstride + min(r0 + SUB, r1)];
  }
  for (int r = r0; r < r1;) {
    int nsub = min(SUB, r1 - r);
    auto scan_counts = [&](int &cnt_, int &excl_, int &n_tot_) __attribute__((always_inline)) {
      cnt_ = (int)(my_hi - my_lo);
      int incl = cnt_;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
      }
      excl_ = incl - cnt_;
      n_tot_ = __builtin_amdgcn_readlane(incl, 63);
    };
    int cnt, excl, n_tot;
    scan_counts(cnt, excl, n_tot);
    while (n_tot > kCandCap && nsub > 1) {  // the super-range overflows LDS: halve it
      nsub >>= 1;
      if (tail) my_hi = bounds[(int64_t)my_i * bstride + r + nsub];
      scan_counts(cnt, excl, n_tot);
    }
#if K2A_TRACE
    tr_post += (uint64_t)n_tot;
#endif
    int64_t nx_hi = my_hi;
    if (r + nsub < r1 && tail) nx_hi = bounds[(int64_t)my_i * bstride + min(r + nsub + SUB, r1)];
    uint64_t Tv = kEmptyKey;
    if (lane < nqw) Tv = __hip_atomic_load(thr_key + q0 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane < kQPerWave) s_tq[wave][lane] = Tv == kEmptyKey ? -INFINITY : f64_unorder(~Tv);  // no T yet: no bound
    if (n_tot > kCandCap) {  // too many tail postings: K2 re-scores these ranges for the wave's queries
      if (lane < nsub) need[(int64_t)qg * nr + r + lane] = (uint8_t)qokm;
      if (lane < nqw * nsub) {  // empty lists (sentinel in slot 0) until K2 re-scores them
        const int qq = lane / nsub, sb = lane - qq * nsub;
        if ((qokm >> qq) & 1u) {
          const int64_t o = lhead(q0 + qq, r + sb, nr);
          cand_key[o] = kEmptyKey;
          cand_row[o] = 0xffffffffu;
        }
      }
      my_lo = my_hi;
      my_hi = nx_hi;
      r += nsub;
      continue;
    }
    if (lane < nsub) need[(int64_t)qg * nr + r + lane] = 0;
    soff[lane] = excl;
    scnt[lane] = cnt;
    // ---- the range's tail postings of the wave's queries -> LDS (list-major, doc-sorted)
    for (int e0 = 0; e0 < n_tot; e0 += 64) {
      const int e = e0 + lane;
      int lo = 0, hi = 63;  // last lane whose exclusive offset <= e (empty lists share offsets)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (__shfl(excl, mid) <= e) lo = mid;
        else hi = mid - 1;
      }
      const int64_t src = __shfl(my_lo, lo) + (e - __shfl(excl, lo));
      if (e < n_tot) {
        pdoc[e] = post_doc[src];
        ptf[e] = (uint16_t)post_tf[src];
        eln[e] = (uint8_t)lo;
      }
    }
    wave_lds_sync();
    // ---- exact score of every candidate, once per query (at its first tail term)
    for (int e0 = 0; e0 < ((dbg & 16) ? 0 : n_tot); e0 += 64) {
      const int e = e0 + lane;
      if (e >= n_tot) break;
      uint64_t key = kEmptyKey;
      const int ln = eln[e];
      const int qb = ln & ~(kTermLanes - 1), j = ln & (kTermLanes - 1);
      const int32_t d = pdoc[e];
      const int32_t tj = st[ln];
      const uint32_t aw = allow ? allow[d >> 5] : 0xffffffffu;
      bool own = (dbg & 512) ? true : (((live[d >> 5] & aw) >> (d & 31)) & 1u);
      for (int jj = 0; jj < j && own; ++jj) {
        const int l2 = qb + jj;
        const int32_t t2 = st[l2];
        if (t2 == tj) own = false;
        else if (!(dbg & 128) && scnt[l2] > 0 && lds_find(pdoc + soff[l2], scnt[l2], d) >= 0) own = false;
      }
      if (own) {
        // the 16 term tf values as 16-bit halves of 8 registers (head bytes land by d16 loads, tail
        // tf are u16): half the VGPRs of one register per term.  Every candidate's head tf bytes
        // and length are gathered up front; the fp32 upper bound follows: below T the exact score
        // is too, and the compaction below would drop the candidate anyway (same T)
        u16x2_t tfp[kTermLanes / 2];
#pragma unroll
        for (int jj = 0; jj < kTermLanes; ++jj) {  // head tf bytes: independent loads, issued together
          const int32_t hh = sh[qb + jj];
          tfp[jj >> 1][jj & 1] =
              hh >= 0 ? ((dbg & 64) ? (uint16_t)1 : (uint16_t)headtf[(int64_t)hh * npad + d]) : (uint16_t)0;
        }
        auto tf_get = [&](int jj) __attribute__((always_inline)) -> uint32_t { return tfp[jj >> 1][jj & 1]; };
        auto tf_set = [&](int jj, uint32_t v) __attribute__((always_inline)) { tfp[jj >> 1][jj & 1] = (uint16_t)v; };
        const int32_t dlen = (dbg & 512) ? 120 : dl[d];
#pragma unroll
        for (int jj = 0; jj < kTermLanes; ++jj) {  // tail terms' tf from the LDS lists
          const int l2 = qb + jj;
          const int32_t t2 = st[l2];
          if (t2 < 0 || sh[l2] >= 0) continue;
          if (t2 == tj) {
            tf_set(jj, ptf[e]);
          } else {
            const int c = (dbg & 256) ? 0 : scnt[l2];
            if (c > 0) {
              const int o = soff[l2];
              const int xx = lds_find(pdoc + o, c, d);
              if (xx >= 0) tf_set(jj, ptf[o + xx]);
            }
          }
        }
        const double Tq = s_tq[wave][qb / kTermLanes];
        float ub = 0.0f;
        const float kd32 = kd_lo32(dlen, inv_avg);
#pragma unroll
        for (int jj = 0; jj < kTermLanes; ++jj)
          if (tf_get(jj)) ub += s_fi[wave][qb + jj] * ratio_up32(tf_get(jj), kd32);
        const bool pass = !((double)(ub * kPlanSlack) < Tq);
        if (pass) {
          const double kd = kd_of(dlen, avgdl);
          double sc = 0.0;
#pragma unroll
          for (int jj = 0; jj < kTermLanes; ++jj) {  // rank_bm25's order: query terms in order
            const int l2 = qb + jj;
            if (st[l2] < 0) continue;  // unknown term / no term: idf 0 -> adds nothing
            if (tf_get(jj)) sc = sc + bm25_contrib_fast(sidf[l2], tf_get(jj), kd);
          }
          key = score_key(sc);
        }
      }
      skey[e] = key;
    }
    wave_lds_sync();
    // ---- top-k of each (range, query).  Entries above their query's global threshold T cannot
    // enter the top-k: drop them and compact the rest in place (key, row, query).
    int n_v = 0;
    for (int e0 = 0; e0 < ((dbg & 32) ? 0 : n_tot); e0 += 64) {
      const int e = e0 + lane;
      uint64_t key = kEmptyKey;
      uint32_t row = 0xffffffffu;
      int qe = 0, ge = 0;
      if (e < n_tot) {
        key = skey[e];
        row = (uint32_t)pdoc[e];
        qe = eln[e] >> 4;
        ge = qe * SUB + ((int)row / kRange - r);  // (query, range) group
      }
      const uint64_t Tq = (uint64_t)__shfl((long long)Tv, qe);  // every lane takes part
      const bool valid = key != kEmptyKey && key <= Tq;
      const uint64_t vm = __ballot(valid);
      const int pos = n_v + (int)__popcll(vm & ((1ull << lane) - 1ull));
      if (valid) {  // pos <= e: this iteration's reads are done, later entries lie above e0 + 63
        skey[pos] = key;
        pdoc[pos] = (int32_t)row;
        eln[pos] = (uint8_t)ge;
      }
      n_v += (int)__popcll(vm);
    }
    wave_lds_sync();
    int cq = 0;  // lane gg < NG: entries written to (query, range) group gg's list
    if (n_v <= 64) {
      // rank = number of entries of the same group with a smaller (key, row): slot index
      const bool mine = lane < n_v;
      const uint64_t key = mine ? skey[lane] : kEmptyKey;
      const uint32_t row = mine ? (uint32_t)pdoc[lane] : 0xffffffffu;
      const int ge = mine ? eln[lane] : 255;
      int rank = 0;
      for (int xx = 0; xx < n_v; ++xx) {  // uniform: LDS broadcast reads
        const int gx = eln[xx];
        rank += (gx == ge && pk_less(skey[xx], (uint32_t)pdoc[xx], key, row)) ? 1 : 0;
        cq += gx == lane ? 1 : 0;
      }
      cq = min(cq, k);
      if (mine && rank < k) {
        const int qe = ge / SUB;
        const int64_t o = lslot(q0 + qe, r + (ge - qe * SUB), nr, lheads_total(nq, nr), k, rank);
        cand_key[o] = key;
        cand_row[o] = row;
        if (rank == k - 1) atomicMin(thr_key + q0 + qe, (unsigned long long)key);  // k entries <= key
      }
    } else {
      // many survivors (a dense generator list before T is known): per-group tournament (rolled:
      // 16 unrolled copies of it cost the main loop registers)
#pragma unroll 1
      for (int gg = 0; gg < NG; ++gg) {
        const int qq = gg / SUB, sb = gg - qq * SUB;
        if (qq >= nqw || sb >= nsub) continue;
        const int qi = q0 + qq;
        uint64_t bk;
        uint32_t br;
        int be;
        auto lane_best = [&]() {
          bk = kEmptyKey;
          br = 0xffffffffu;
          be = -1;
          for (int e = lane; e < n_v; e += 64) {
            if (eln[e] != gg) continue;
            const uint64_t kk = skey[e];
            if (kk == kEmptyKey) continue;
            const uint32_t rr = (uint32_t)pdoc[e];
            if (pk_less(kk, rr, bk, br)) {
              bk = kk;
              br = rr;
              be = e;
            }
          }
        };
        lane_best();
        int i = 0;
        uint64_t last = kEmptyKey;
        for (; i < k; ++i) {
          uint64_t mk = bk;
          uint32_t mr = br;
          wave_min_pair(mk, mr);
          if (mr == 0xffffffffu) break;
          if (lane == 0) {
            const int64_t o = lslot(qi, r + sb, nr, lheads_total(nq, nr), k, i);
            cand_key[o] = mk;
            cand_row[o] = mr;
          }
          last = mk;
          if (br == mr && bk == mk) {
            skey[be] = kEmptyKey;
            lane_best();
          }
        }
        if (lane == gg) cq = i;
        if (i == k && lane == 0) atomicMin(thr_key + qi, (unsigned long long)last);
      }
    }
    // terminate each list after its entries (one sentinel at slot = count; readers stop there):
    // lane gg holds group gg's count
    static_assert(NG <= 64, "one lane per (query, range) group");
    if (lane < NG) {
      const int qq = lane / SUB, sb = lane - qq * SUB;
      if (qq < nqw && sb < nsub && ((qokm >> qq) & 1u) && cq < k) {
        const int64_t o = lslot(q0 + qq, r + sb, nr, lheads_total(nq, nr), k, cq);
        cand_key[o] = kEmptyKey;
        cand_row[o] = 0xffffffffu;
      }
    }
    wave_lds_sync();  // LDS slice reused by the next range
    my_lo = my_hi;
    my_hi = nx_hi;
    r += nsub;
  }
#if K2A_TRACE
  if (lane == 0) {
    uint64_t *tr = g_k2a_trace + 4 * (int64_t)wid;
    const uint64_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;  // XCC_ID[3:0]
    tr[0] = (xcc << 32) | (uint64_t)(wid + 1);
    tr[1] = tr_t0;
    tr[2] = __builtin_amdgcn_s_memrealtime();
    tr[3] = tr_post;
  }
#endif
}

// Re-score planning after the tail pass.  top_score / top_row are the merged tail-pass lists,
// so T = top_score[q][k-1] is the k-th best tail score of query q.  One thread per (query
// group qg, range r):
//  * need[qg * nr + r] bit qq -> K2 re-scores the whole range: the tail pass's overflow bits,
//    and every range of a query with more than kTermLanes terms or without a positive T;
//  * otherwise, when the range-level head-only bound reaches T, the 16 block-level (64-doc)
//    bounds pick the blocks K2b scores: item = q << 40 | r << 16 | block mask (appended
//    wave-aggregated at items[*item_count]).
// The bounds only choose what gets scored, so they are computed in fp32 and inflated by
// kPlanSlack (>> the < 1e-6 relative rounding of <= 16 fp32 terms): a pair is dropped only when
// even the inflated bound is below T.  Term descriptors come from qd_* (one load level: the
// head id, walked flag and idf of all 16 slots at once), the per-(head, range) maxima after them.
__global__ void __launch_bounds__(256)
    bm25_plan_kernel(const int32_t *__restrict__ qd_code, const double *__restrict__ qd_idf,
                     const int32_t *__restrict__ qd_len, int nq, int has_heads,
                     const uint8_t *__restrict__ head_maxtf, const int32_t *__restrict__ range_mindl,
                     const uint8_t *__restrict__ blk_maxtf, const int32_t *__restrict__ blk_mindl,
                     const uint8_t *__restrict__ blk_maxr, double maxr_avgdl, int nr,
                     int64_t nblk, const double *__restrict__ avgdl_p, int k, const double *__restrict__ top_score,
                     const int64_t *__restrict__ top_row, uint8_t *__restrict__ need, uint64_t *__restrict__ items,
                     uint32_t *__restrict__ item_count, const uint8_t *__restrict__ blk16_maxr,
                     uint64_t *__restrict__ items_sm) {
  const double avgdl = *avgdl_p;
  const bool use_r = blk_maxr != nullptr && avgdl <= maxr_avgdl;  // the stored ratio bound is valid
  const float inv_avg = inv_avg_lo(avgdl);
  auto kd_lo = [&](int32_t dlen) __attribute__((always_inline)) { return kd_lo32(dlen, inv_avg); };
  const int nqg = (nq + kQPerWave - 1) / kQPerWave;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = gid < (int64_t)nqg * nr;  // inactive threads still join the wave's append
  const int lane = threadIdx.x & 63;
  uint64_t it[kQPerWave], its[kQPerWave];
  int nit = 0;
  if (act) {
    const int qg = (int)(gid / nr), r = (int)(gid - (int64_t)qg * nr);
    uint32_t m = need[gid];
    const float kd = kd_lo(range_mindl[r]);
    for (int qq = 0; qq < kQPerWave; ++qq) {
      const int q = qg * kQPerWave + qq;
      if (q >= nq) break;
      const uint32_t bit = 1u << qq;
      if (m & bit) continue;
      const double T = top_score[(int64_t)q * k + k - 1];
      if (qd_len[q] > kTermLanes || top_row[(int64_t)q * k + k - 1] < 0 || !(T > 0.0)) {
        m |= bit;
        continue;
      }
      if (!has_heads) continue;  // no head terms: every scoring document is a tail candidate
      // the query's bounded head slots: head, not walked (generators' documents are all tail
      // candidates), positive idf
      int32_t hs[kTermLanes];
      float fi[kTermLanes];
      uint32_t mt[kTermLanes];
      {
        const int4 *cp = reinterpret_cast<const int4 *>(qd_code + (int64_t)q * kTermLanes);
        const double2 *ip = reinterpret_cast<const double2 *>(qd_idf + (int64_t)q * kTermLanes);
#pragma unroll
        for (int v = 0; v < kTermLanes / 4; ++v) {
          const int4 c4 = cp[v];
          hs[4 * v] = c4.x;
          hs[4 * v + 1] = c4.y;
          hs[4 * v + 2] = c4.z;
          hs[4 * v + 3] = c4.w;
        }
#pragma unroll
        for (int v = 0; v < kTermLanes / 2; ++v) {
          const double2 f2 = ip[v];
          fi[2 * v] = idf_up(f2.x);
          fi[2 * v + 1] = idf_up(f2.y);
        }
      }
#pragma unroll
      for (int j = 0; j < kTermLanes; ++j) {
        const int32_t c = hs[j];
        hs[j] = ((c >> 30) & 1) || !(fi[j] > 0.0f) ? -1 : (c & 0x3fffffff) - 1;
        mt[j] = hs[j] >= 0 ? head_maxtf[(int64_t)hs[j] * nr + r] : 0u;  // issued together
      }
      float ub = 0.0f;
#pragma unroll
      for (int j = 0; j < kTermLanes; ++j)
        if (mt[j]) {
          const float tf = (float)mt[j];
          ub += fi[j] * ((tf * 2.5f) / (tf + kd));
        }
      if ((double)(ub * kPlanSlack) < T) continue;
      // block level: 16 blocks of 64 documents
      float kdb[16], ubb[16];
      {
        const int4 *md = reinterpret_cast<const int4 *>(blk_mindl + (int64_t)r * 16);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int4 x4 = md[v];
          kdb[4 * v] = kd_lo(x4.x);
          kdb[4 * v + 1] = kd_lo(x4.y);
          kdb[4 * v + 2] = kd_lo(x4.z);
          kdb[4 * v + 3] = kd_lo(x4.w);
        }
      }
      // sub-block level (round 6): the same sum over the 16-doc sub-blocks' stored ratio maxima, each
      // head's term capped by its block bound -- the planned blocks' documents almost never reach T
      // (15 of 76 M at the bench shape, profiles/r06_k2b_stat.txt), and 95 % of their sub-blocks are
      // below it: K2b then reads only the planned sub-blocks
      const bool use_s = use_r && blk16_maxr != nullptr;
      float ubs[64];
#pragma unroll
      for (int b = 0; b < 16; ++b) ubb[b] = 0.0f;
#pragma unroll
      for (int x = 0; x < 64; ++x) ubs[x] = 0.0f;
      for (int j = 0; j < kTermLanes; ++j) {
        if (!mt[j]) continue;
        const int32_t hh = hs[j];
        const uint4 v4 = *reinterpret_cast<const uint4 *>(blk_maxtf + (int64_t)hh * nblk + (int64_t)r * 16);
        const uint32_t wv[4] = {v4.x, v4.y, v4.z, v4.w};
        uint32_t rv[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        if (use_r) {
          const uint4 r4 = *reinterpret_cast<const uint4 *>(blk_maxr + (int64_t)hh * nblk + (int64_t)r * 16);
          rv[0] = r4.x;
          rv[1] = r4.y;
          rv[2] = r4.z;
          rv[3] = r4.w;
        }
        uint32_t sv[16];
        if (use_s) {
          const uint4 *sp = reinterpret_cast<const uint4 *>(blk16_maxr + ((int64_t)hh * nblk + (int64_t)r * 16) * 4);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const uint4 s4 = sp[v];
            sv[4 * v] = s4.x;
            sv[4 * v + 1] = s4.y;
            sv[4 * v + 2] = s4.z;
            sv[4 * v + 3] = s4.w;
          }
        }
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          const uint32_t bt = (wv[b >> 2] >> (8 * (b & 3))) & 0xffu;
          if (bt) {
            // two upper bounds of the head's ratio in this block: (max tf, shortest document) and
            // the stored per-document maximum (quantised upwards, q / 102 > max ratio)
            const float tf = (float)bt;
            float rb = (tf * 2.5f) / (tf + kdb[b]);
            if (use_r) rb = fminf(rb, (float)((rv[b >> 2] >> (8 * (b & 3))) & 0xffu) * (1.0f / 102.0f));
            ubb[b] += fi[j] * rb;
            if (use_s) {   // sub-block s of block b: byte s of word b (a zero byte: the head is absent there)
#pragma unroll
              for (int x = 0; x < 4; ++x)
                ubs[4 * b + x] += fi[j] * fminf(rb, (float)((sv[b] >> (8 * x)) & 0xffu) * (1.0f / 102.0f));
            }
          }
        }
      }
      uint32_t bm = 0;
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if ((double)(ubb[b] * kPlanSlack) >= T) bm |= 1u << b;
      uint64_t sm = 0;   // planned 16-doc sub-blocks (4 b + x)
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        if (!((bm >> b) & 1u)) continue;
        if (!use_s) {
          sm |= 0xfull << (4 * b);
          continue;
        }
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if ((double)(ubs[4 * b + x] * kPlanSlack) >= T) sm |= 1ull << (4 * b + x);
      }
      uint32_t bms = 0;  // blocks holding a planned sub-block (the postings walk marks their documents)
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if ((sm >> (4 * b)) & 0xfull) bms |= 1u << b;
      if (bms) {
        its[nit] = sm;
        it[nit++] = ((uint64_t)q << 40) | ((uint64_t)r << 16) | bms;
      }
    }
    need[gid] = (uint8_t)m;
  }
  // wave-aggregated append of the items
  int incl = nit;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o);
    if (lane >= o) incl += v;
  }
  const int total = __shfl(incl, 63);
  if (total == 0) return;
  uint32_t base = 0;
  if (lane == 63) base = atomicAdd(item_count, (uint32_t)total);
  base = (uint32_t)__shfl((int)base, 63);
  for (int i = 0; i < nit; ++i) {
    items[base + (uint32_t)(incl - nit + i)] = it[i];
    items_sm[base + (uint32_t)(incl - nit + i)] = its[i];
  }
}

// true when the fp32 upper bound of a head-only document's score (its head terms' tf bytes,
// idf rounded up per lane j = term slot, K_d bounded below) is below T: its exact score is too
// (headm: the item's head slots, wave-uniform.  Only those slots hold tf bytes, and a zero byte adds
// fi . ratio_up32(0, kd) = +0.0 exactly, so the uniform skip of the other slots and the branch-free
// add give the bits of the per-lane `if (tfv[j])` form without its 16 exec-mask branches per block)
__device__ inline bool k2b_below(const uint32_t (&tfv)[kTermLanes], float fi, float kd, double T, uint64_t headm) {
  float ub = 0.0f;
#pragma unroll
  for (int j = 0; j < kTermLanes; ++j)
    if ((headm >> j) & 1u) ub += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fi), j)) * ratio_up32(tfv[j], kd);
  return (double)(ub * kPlanSlack) < T;
}

// K2b's per-wave list of documents at or above T: compacted to the k best whenever fewer than 64
// free slots remain (k <= kMaxTopK, so a compaction always frees >= 64)
constexpr int kK2bCap = kMaxTopK + 64;
static_assert(kK2bCap / 64 * 64 == kK2bCap, "whole wave chunks");
__device__ inline int k2b_compact(uint64_t *ckey, uint32_t *crow, int n, int k, int lane) {
  constexpr int C = kK2bCap / 64;
  uint64_t kk[C];
  uint32_t rr[C];
  int rk[C];
  wave_lds_sync();  // the appends of every lane
#pragma unroll
  for (int c = 0; c < C; ++c) {  // all reads before any write (the writes land in slots < k)
    const int e = lane + 64 * c;
    rk[c] = kMaxTopK;
    if (e < n) {
      kk[c] = ckey[e];
      rr[c] = crow[e];
      int rank = 0;
      for (int x = 0; x < n; ++x) rank += pk_less(ckey[x], crow[x], kk[c], rr[c]) ? 1 : 0;
      rk[c] = rank;
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (rk[c] < k) {
      ckey[rk[c]] = kk[c];
      crow[rk[c]] = rr[c];
    }
  wave_lds_sync();
  return min(n, k);
}

// K2b: exact scores of the head-only documents of the planned 64-doc blocks, merged into the
// (query, range) list of the tail pass.  The two sets are disjoint — a document holding a tail
// query term is skipped here (the tail pass scored it) — so the list's top-k stays exact.  A
// head-only document's score is the query-order sum of its head-term contributions (tail terms
// add idf * 0), bit-identical to K2's.  One wave per item, grid-stride over *item_count.
// Latency structure: a wave's next item and its query's descriptors (qd_*, built by
// bm25_qcand_kernel) are loaded while the current item is scored, and the first blocks' tile
// loads are issued before the walk over the tail postings of the range, so an item costs about
// two dependent load levels (bounds -> postings, tiles) instead of five.
#ifndef K2B_WPE
#define K2B_WPE 4
#endif
#ifndef K2B_ABL  // timing ablations (variant builds only; results invalid): 1 no postings walk,
#define K2B_ABL 0  // 2 no tile loads, 4 no scoring, 8 no block work at all, 16 integer sum for
// the fp64 scoring, 32 scoring without the merge, 64 no fp32 pre-bound
#endif
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(K2B_WPE)))
    bm25_block_kernel(const uint64_t *__restrict__ items, const uint32_t *__restrict__ item_count,
                      const int32_t *__restrict__ qd_code, const double *__restrict__ qd_idf,
                      const int32_t *__restrict__ qd_tb, const int64_t *__restrict__ bounds, int nr,
                      const int32_t *__restrict__ post_doc, const uint8_t *__restrict__ headtf, int64_t npad,
                      const int32_t *__restrict__ dl, const uint32_t *__restrict__ live,
                      const uint32_t *__restrict__ allow, int64_t ndocs, const double *__restrict__ avgdl_p, int k,
                      const double *__restrict__ top_score, int nq, uint64_t *__restrict__ cand_key,
                      uint32_t *__restrict__ cand_row, const uint64_t *__restrict__ items_sm) {
  constexpr int W = 4;
  const double avgdl = *avgdl_p;
  __shared__ uint64_t s_tmask[W][16];
  __shared__ uint64_t s_ckey[W][kK2bCap], s_tkey[W][kMaxTopK];
  __shared__ uint32_t s_crow[W][kK2bCap], s_trow[W][kMaxTopK];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const uint32_t n_items = *item_count;
  const uint32_t stride = gridDim.x * W;
  uint32_t itx = blockIdx.x * W + wave;
  if (itx >= n_items) return;  // whole wave
  const int tl = lane < kTermLanes ? lane : 0;
  const float inv_avg = inv_avg_lo(avgdl);
  uint64_t *ckey = s_ckey[wave], *tkey = s_tkey[wave];
  uint32_t *crow = s_crow[wave], *trow = s_trow[wave];
  uint64_t item = items[itx], item_sm = items_sm[itx];
  int q = (int)(item >> 40);
  int32_t code = lane < kTermLanes ? qd_code[(int64_t)q * kTermLanes + tl] : 0;
  double idf = lane < kTermLanes ? qd_idf[(int64_t)q * kTermLanes + tl] : 0.0;
  int tb = qd_tb[q];
  double Tsc = top_score[(int64_t)q * k + k - 1];
  for (;;) {
    const uint32_t nitx = itx + stride;
    const bool has_next = nitx < n_items;  // wave-uniform
    const uint64_t nitem = has_next ? items[nitx] : 0;
    const uint64_t nitem_sm = has_next ? items_sm[nitx] : 0;
    const int r = (int)((item >> 16) & 0xffffffu);
    const uint32_t bm = (uint32_t)(item & 0xffffu);
    const int64_t d0 = (int64_t)r * kRange;
    const int32_t hh = (code & 0x3fffffff) - 1;
    const bool walked = (code >> 30) & 1;
    const uint64_t headm = __ballot(hh >= 0);
    int64_t plo = 0, phi = 0;
    if (walked) {
      plo = bounds[(int64_t)(tb + lane) * (nr + 1) + r];
      phi = bounds[(int64_t)(tb + lane) * (nr + 1) + r + 1];
    }
    if (lane < 16) s_tmask[wave][lane] = 0;
    // the planned blocks, K2B_U at a time: every load of the group (head tf bytes, length, live /
    // allow words; clamped, unconditional) is issued before any arithmetic, so a wave keeps
    // K2B_U blocks' loads in flight instead of one dependent chain per block
    // the planned 16-doc sub-blocks (round 6), four per 64-lane unit: lane group l >> 4 takes the
    // unit's (l >> 4)-th sub-block, lane l & 15 its document (-1: fewer than four left)
    uint64_t mb = (K2B_ABL & 8) ? 0ull : item_sm;
    int bq[K2B_U];     // per unit: this lane's sub-block (0..63) or -1
    int nbq = 0;
    uint32_t tfv[K2B_U][kTermLanes];
    uint32_t lwv[K2B_U], awv[K2B_U];
    int32_t dlv[K2B_U];
    auto load_group = [&]() __attribute__((always_inline)) {
      nbq = 0;
#pragma unroll
      for (int u = 0; u < K2B_U; ++u) {
        int pick = -1;
#pragma unroll
        for (int x = 0; x < 4; ++x) {   // wave-uniform: the next four set bits
          const int sb = mb ? (int)__builtin_ctzll(mb) : -1;
          if (mb) mb &= mb - 1;
          if ((lane >> 4) == x) pick = sb;
          if (x == 0 && sb >= 0) ++nbq;
        }
        bq[u] = pick;
      }
#pragma unroll
      for (int u = 0; u < K2B_U; ++u) {
        const int64_t d = d0 + max(bq[u], 0) * 16 + (lane & 15);
        const int64_t dc = d < ndocs ? d : ndocs - 1;
#pragma unroll
        for (int j = 0; j < kTermLanes; ++j) {  // head tf bytes (tiles are padded to whole ranges)
          tfv[u][j] = 0u;
          if (((headm >> j) & 1u) && u < nbq)
            tfv[u][j] = (K2B_ABL & 2) ? 1u : headtf[(int64_t)__builtin_amdgcn_readlane(hh, j) * npad + d];
        }
        lwv[u] = live[dc >> 5];
        awv[u] = allow ? allow[dc >> 5] : 0xffffffffu;
        dlv[u] = dl[dc];
      }
    };
    load_group();  // in flight during the postings walk below
    wave_lds_sync();
    // documents of the planned blocks that hold a tail query term
    for (uint64_t tm = (K2B_ABL & 1) ? 0 : __ballot(phi > plo); tm; tm &= tm - 1) {
      const int j = __builtin_ctzll(tm);
      const int64_t lo = (int64_t)readlane_u64((uint64_t)plo, j), hi = (int64_t)readlane_u64((uint64_t)phi, j);
      for (int64_t p = lo + lane; p < hi; p += 64) {
        const int off = post_doc[p] - (int32_t)d0;
        const int b = off >> 6;
        if ((bm >> b) & 1u) atomicOr(&s_tmask[wave][b], 1ull << (off & 63));
      }
    }
    wave_lds_sync();
    // the next item's query descriptors (its item word has arrived by now)
    int32_t ncode = 0;
    double nidf = 0.0, nT = 0.0;
    int ntb = 0;
    if (has_next) {
      const int nq_ = (int)(nitem >> 40);
      if (lane < kTermLanes) {
        ncode = qd_code[(int64_t)nq_ * kTermLanes + tl];
        nidf = qd_idf[(int64_t)nq_ * kTermLanes + tl];
      }
      ntb = qd_tb[nq_];
      nT = top_score[(int64_t)nq_ * k + k - 1];
    }
    const uint64_t Tk = score_key(Tsc);
    const float fi = idf_up(idf);  // lane j: term slot j's idf, rounded up (0 when <= 0)
    int n = 0;  // documents of the planned blocks at or above T, appended to the wave's c list
    for (;;) {
#pragma unroll
      for (int u = 0; u < K2B_U; ++u) {
        if (u >= nbq) break;
        const int sb = bq[u];
        const int64_t d = d0 + max(sb, 0) * 16 + (lane & 15);
        uint64_t key = kEmptyKey;
        const bool ok = sb >= 0 && d < ndocs && !((s_tmask[wave][sb >> 2] >> (((sb & 3) << 4) | (lane & 15))) & 1u) &&
                        (((lwv[u] & awv[u]) >> (d & 31)) & 1u);
        if (ok && (K2B_ABL & 16)) {  // loads kept, integer sum instead of the fp64 scoring
          uint32_t t = (uint32_t)dlv[u];
#pragma unroll
          for (int j = 0; j < kTermLanes; ++j) t += tfv[u][j];
          key = t == 0xfffffffu ? 0ull : kEmptyKey;
        } else if (ok && !(K2B_ABL & 4) && ((K2B_ABL & 64) || !k2b_below(tfv[u], fi, kd_lo32(dlv[u], inv_avg), Tsc, headm))) {
          // exact fp64 score only where the fp32 upper bound reaches T (a few documents per
          // query: the bound's slack is 2e-5 relative, the planned blocks' documents mostly fall
          // far below T)
          const double kd = kd_of(dlv[u], avgdl);
          double sc = 0.0;
#pragma unroll
          for (int j = 0; j < kTermLanes; ++j)   // (non-head slots hold no tf: skipped wave-uniformly)
            if (((headm >> j) & 1u) && tfv[u][j]) sc = sc + bm25_contrib_fast(readlane_f64(idf, j), tfv[u][j], kd);
          key = score_key(sc);
          if ((K2B_ABL & 32) && sc > -1.0) key = kEmptyKey;  // never merges
        }
        const bool pass = key <= Tk;  // at or above the query's k-th best tail score
        const uint64_t pm = __ballot(pass);
        if (pass) {
          const int pos = n + (int)__popcll(pm & ((1ull << lane) - 1ull));
          ckey[pos] = key;
          crow[pos] = (uint32_t)d;
        }
        n += (int)__popcll(pm);
        if (n > kK2bCap - 64) n = k2b_compact(ckey, crow, n, k, lane);  // keep the k best
      }
      if (!mb) break;
      load_group();
    }
    // merge with the tail pass's (sorted) list of (q, r) by ranks: the two sets are disjoint, so
    // every (key, row) is distinct and the ranks over their union are a permutation (nothing to
    // do when no document of the planned blocks reached T: the common case)
    if (n > 0) {
      const int64_t nl = lheads_total(nq, nr);
      wave_lds_sync();
      // the list's entries end at its sentinel (slots past it hold stale data): nt = first empty slot
      int nt = k;
      for (int i0 = 0; i0 < k && nt == k; i0 += 64) {  // wave-uniform
        const int i = i0 + lane;
        uint32_t rr = 0xffffffffu;
        if (i < k) {
          rr = cand_row[lslot(q, r, nr, nl, k, i)];
          tkey[i] = cand_key[lslot(q, r, nr, nl, k, i)];
          trow[i] = rr;
        }
        const uint64_t em = __ballot(i < k && rr == 0xffffffffu);
        if (em) nt = i0 + __builtin_ctzll(em);
      }
      wave_lds_sync();
      // ranks of the new entries (among both sets) and of the list's entries (among the new ones)
      for (int e = lane; e < n; e += 64) {
        const uint64_t kk = ckey[e];
        const uint32_t rr = crow[e];
        int rank = 0;
        for (int x = 0; x < n; ++x) rank += pk_less(ckey[x], crow[x], kk, rr) ? 1 : 0;
        for (int x = 0; x < nt; ++x) rank += pk_less(tkey[x], trow[x], kk, rr) ? 1 : 0;
        if (rank < k) {
          cand_key[lslot(q, r, nr, nl, k, rank)] = kk;
          cand_row[lslot(q, r, nr, nl, k, rank)] = rr;
        }
      }
      for (int i = lane; i < nt; i += 64) {
        const uint64_t kk = tkey[i];
        const uint32_t rr = trow[i];
        int rank = i;
        for (int x = 0; x < n; ++x) rank += pk_less(ckey[x], crow[x], kk, rr) ? 1 : 0;
        if (rank < k) {
          cand_key[lslot(q, r, nr, nl, k, rank)] = kk;
          cand_row[lslot(q, r, nr, nl, k, rank)] = rr;
        }
      }
      if (lane == 0 && n + nt < k) {  // new terminator
        cand_key[lslot(q, r, nr, nl, k, n + nt)] = kEmptyKey;
        cand_row[lslot(q, r, nr, nl, k, n + nt)] = 0xffffffffu;
      }
    }
    wave_lds_sync();  // LDS reused by the next item
    if (!has_next) break;
    itx = nitx;
    item = nitem;
    item_sm = nitem_sm;
    q = (int)(item >> 40);
    code = ncode;
    idf = nidf;
    tb = ntb;
    Tsc = nT;
  }
}

// blk_maxtf[h * nblk + b] = largest tf byte of head term h in 64-doc block b.
// Per (head, 64-doc block): the largest ratio tf.2.5/(tf + K_d) of the block's documents at the given
// avgdl, stored as q = floor(ratio . 102) + 1 (so q / 102 > the ratio; ratio < 2.5 -> q <= 255).
// (bs = 64: blk_maxr, the planner's block level; bs = 16: blk16_maxr, its 16-doc sub-block level)
__global__ void bm25_blk_maxratio_kernel(const uint8_t *__restrict__ headtf, int64_t npad,
                                         const int32_t *__restrict__ dl, int64_t ndocs, int64_t nblk, int nhead,
                                         double avgdl, uint8_t *__restrict__ blk_maxr, int bs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nhead * nblk) return;
  const int64_t hh = i / nblk, b = i - hh * nblk;
  double m = 0.0;
  for (int u = 0; u < bs; ++u) {
    const int64_t d = b * bs + u;
    if (d >= ndocs) break;
    const uint32_t tf = headtf[hh * npad + d];
    if (!tf) continue;
    const double t = (double)tf;
    m = fmax(m, (t * 2.5) / (t + kd_of(dl[d], avgdl)));
  }
  blk_maxr[i] = m > 0.0 ? (uint8_t)min(255.0, floor(m * 102.0) + 1.0) : (uint8_t)0;
}

__global__ void bm25_blk_max_kernel(const uint8_t *__restrict__ headtf, int64_t npad, int64_t nblk, int nhead,
                                    uint8_t *__restrict__ blk_maxtf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nhead * nblk) return;
  const int64_t hh = i / nblk, b = i - hh * nblk;
  const uint4 *p = reinterpret_cast<const uint4 *>(headtf + hh * npad + b * 64);
  uint32_t m = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const uint4 x4 = p[v];
    const uint32_t wv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t a = wv[u];
      m = max(m, max(max(a & 0xffu, (a >> 8) & 0xffu), max((a >> 16) & 0xffu, a >> 24)));
    }
  }
  blk_maxtf[i] = (uint8_t)m;
}

// blk_mindl[b] = shortest document length in 64-doc block b (INT32_MAX past the last document).
__global__ void bm25_blk_mindl_kernel(const int32_t *__restrict__ dl, int64_t ndocs, int64_t nblk,
                                      int32_t *__restrict__ blk_mindl) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblk) return;
  int32_t m = INT32_MAX;
  for (int u = 0; u < 64; ++u) {
    const int64_t d = b * 64 + u;
    if (d < ndocs) m = min(m, dl[d]);
  }
  blk_mindl[b] = m;
}

// head_maxtf[h * nr + r] = largest tf byte of head term h in range r (one wave per pair).
__global__ void bm25_head_max_kernel(const uint8_t *__restrict__ headtf, int64_t npad, int nr, int nhead,
                                     uint8_t *__restrict__ head_maxtf) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= (int64_t)nhead * nr) return;
  const int lane = threadIdx.x & 63;
  const int64_t hh = w / nr, r = w - hh * nr;
  const uint4 v = *reinterpret_cast<const uint4 *>(headtf + hh * npad + r * kRange + 16 * lane);
  const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t a = wv[u];
    m = max(m, max(max(a & 0xffu, (a >> 8) & 0xffu), max((a >> 16) & 0xffu, a >> 24)));
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if (lane == 0) head_maxtf[w] = (uint8_t)m;
}

// range_mindl[r] = shortest document length in range r (all rows, live or not).
__global__ void bm25_range_mindl_kernel(const int32_t *__restrict__ dl, int64_t ndocs, int nr,
                                        int32_t *__restrict__ range_mindl) {
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= nr) return;
  const int lane = threadIdx.x & 63;
  int32_t m = INT32_MAX;
  for (int u = 0; u < kRange / 64; ++u) {
    const int64_t d = w * kRange + u * 64 + lane;
    if (d < ndocs) m = min(m, dl[d]);
  }
  for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
  if (lane == 0) range_mindl[w] = m;
}

// K2s: a running threshold before the tail pass (round 5).  K2a's T comes from its own lists, so the
// first super-ranges of every query run without one (every candidate survives; the dense survivor
// sets take the per-group tournament).  Here one wave per query scores a sample of real documents --
// the first kSeedCap postings of the query's rarest walked term (live and allowed only) -- with a lower
// bound of their exact score: the walked term's and the head terms' contributions, in query order,
// the other tail terms left out.  With every idf >= 0 each contribution is >= 0 and a sum of fewer
// of them in the same order is <= the full one (IEEE addition is monotone), so k distinct documents
// score >= the k-th smallest bound: its key is a valid K2a threshold (k entries <= key), set by
// atomicMin exactly like a filled list's.  Queries with a negative idf (rank_bm25's epsilon floor
// below zero, quirk Q1), more than kTermLanes terms or fewer than k sampled documents get no seed.
#ifndef K2S_CAP
#define K2S_CAP 1024
#endif
constexpr int kSeedCap = K2S_CAP;   // sampled postings of the rarest walked term per query
constexpr int kSeedThreads = 256;
constexpr int kSeedPer = kSeedCap / kSeedThreads;   // sampled postings per thread
// one 256-thread workgroup per query; each thread scores <= kSeedPer sampled documents with every
// head tf byte and the length loaded up front (independent loads), then k rounds of a block
// tournament over the threads' sorted keys give the k-th smallest bound key
__global__ void __launch_bounds__(kSeedThreads) bm25_tseed_kernel(
    int nq, int k, const int32_t *__restrict__ qd_code, const double *__restrict__ qd_idf,
    const int32_t *__restrict__ qd_len, const int32_t *__restrict__ qd_term, const int64_t *__restrict__ term_off,
    const int32_t *__restrict__ post_doc, const uint16_t *__restrict__ post_tf, const uint8_t *__restrict__ headtf,
    int64_t npad, const int32_t *__restrict__ dl, const uint32_t *__restrict__ live,
    const uint32_t *__restrict__ allow, const double *__restrict__ avgdl_p,
    unsigned long long *__restrict__ thr_key) {
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (q >= nq || k > kSeedCap) return;   // whole workgroup
  const int L = qd_len[q];
  if (L <= 0 || L > kTermLanes) return;
  __shared__ int32_t s_t[kTermLanes], s_h[kTermLanes];
  __shared__ double s_i[kTermLanes];
  __shared__ uint64_t sk[kSeedThreads / 64];
  __shared__ int s_gt, s_bad, s_n;
  __shared__ int64_t s_p0;
  if (wave == 0) {
    int32_t t = -1, code = 0;
    double idf = 0.0;
    if (lane < kTermLanes) {
      if (lane < L) {
        t = qd_term[(int64_t)q * kTermLanes + lane];
        code = qd_code[(int64_t)q * kTermLanes + lane];
        idf = qd_idf[(int64_t)q * kTermLanes + lane];
      }
      s_t[lane] = t;
      s_h[lane] = (code & 0x3fffffff) - 1;
      s_i[lane] = idf;
    }
    const bool bad = __ballot(lane < L && t >= 0 && idf < 0.0) != 0;   // a negative contribution is possible
    // the rarest walked term (lowest df, then lowest slot)
    const bool walked = lane < L && t >= 0 && ((code >> 30) & 1);
    int64_t df = walked ? term_off[t + 1] - term_off[t] : INT64_MAX;
    int best = walked ? lane : 64;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t odf = __shfl_xor(df, o);
      const int ob = __shfl_xor(best, o);
      if (odf < df || (odf == df && ob < best)) {
        df = odf;
        best = ob;
      }
    }
    const int32_t gt_all = __shfl(t, best < 64 ? best : 0);   // every lane takes part
    if (lane == 0) {
      s_bad = bad || best >= 64 || df < k;
      s_gt = best < 64 ? gt_all : -1;
      s_n = (int)min<int64_t>(df, kSeedCap);
      s_p0 = best < 64 ? term_off[gt_all] : 0;
    }
  }
  __syncthreads();
  if (s_bad) return;   // uniform
  const int32_t gt = s_gt;
  const int n = s_n;
  const int64_t p0 = s_p0;
  const double avgdl = *avgdl_p;
  uint64_t kk[kSeedPer];   // this thread's bound keys, sorted (smaller = higher score)
#pragma unroll
  for (int i = 0; i < kSeedPer; ++i) kk[i] = kEmptyKey;
#pragma unroll
  for (int u = 0; u < kSeedPer; ++u) {
    const int e = tid + u * kSeedThreads;
    if (e >= n) break;
    const int32_t d = post_doc[p0 + e];
    const uint32_t tfg = post_tf[p0 + e];
    const uint32_t aw = allow ? allow[d >> 5] : 0xffffffffu;
    const bool ok = ((live[d >> 5] & aw) >> (d & 31)) & 1u;
    const int32_t dlen = dl[d];
    uint32_t tf[kTermLanes];
#pragma unroll
    for (int j = 0; j < kTermLanes; ++j) {   // head tf bytes: independent loads, issued together
      const int32_t h = s_h[j];
      tf[j] = (j < L && h >= 0) ? (uint32_t)headtf[(int64_t)h * npad + d] : 0u;
    }
    if (!ok) continue;
    const double kd = kd_of(dlen, avgdl);
    double sc = 0.0;
#pragma unroll
    for (int j = 0; j < kTermLanes; ++j) {   // rank_bm25's order; duplicates of a term add again
      if (j >= L) break;
      const int32_t tj = s_t[j];
      if (tj < 0) continue;
      const uint32_t v = tj == gt ? tfg : tf[j];   // other tail terms: left out (the lower bound)
      if (v) sc = sc + bm25_contrib_fast(s_i[j], v, kd);
    }
    uint64_t ck = score_key(sc);
#pragma unroll
    for (int i = 0; i < kSeedPer; ++i) {   // sorted insertion, static indices
      if (ck < kk[i]) {
        const uint64_t tmp = kk[i];
        kk[i] = ck;
        ck = tmp;
      }
    }
  }
  // k rounds of a block tournament over the threads' fronts: the k-th pop is the k-th smallest key
  uint64_t kth = kEmptyKey;
  for (int i = 0; i < k; ++i) {
    uint64_t m = kk[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t om = __shfl_xor(m, o);
      m = om < m ? om : m;
    }
    if (lane == 0) sk[wave] = m;
    __syncthreads();
    m = sk[0];
#pragma unroll
    for (int w2 = 1; w2 < kSeedThreads / 64; ++w2) m = sk[w2] < m ? sk[w2] : m;
    __syncthreads();   // sk is rewritten next round
    if (m == kEmptyKey) return;   // fewer than k sampled documents (uniform)
    kth = m;
    // one owner pops: the lowest thread holding m (keys of distinct documents may be equal)
    const uint64_t mine = __ballot(kk[0] == m);
    const int wl = mine ? (int)__builtin_ctzll(mine) : 64;
    if (lane == 0) sk[wave] = (uint64_t)wl;
    __syncthreads();
    int owner = -1;
    for (int w2 = 0; w2 < kSeedThreads / 64; ++w2)
      if (owner < 0 && sk[w2] < 64) owner = w2 * 64 + (int)sk[w2];
    __syncthreads();
    if (tid == owner) {
#pragma unroll
      for (int t2 = 0; t2 + 1 < kSeedPer; ++t2) kk[t2] = kk[t2 + 1];
      kk[kSeedPer - 1] = kEmptyKey;
    }
  }
  if (tid == 0) atomicMin(thr_key + q, (unsigned long long)kth);
}
