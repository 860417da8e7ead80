// The validation metrics that need more than one reduction: AUC-Judd (below), the shuffled AUC and AUC-Borji (second part of the
// file: one prep kernel and one split kernel, split_auc_kernel, with the metric's draw as a template argument) and the information
// gain (last part).
//
// AUC-Judd (loss.py:122-213), the fifth validation metric, as a rank problem: one workgroup (1024 lanes) per map.
//
// The reference sweeps one threshold per fixation over the whole map, O(pixels x fixations).  Here, per map S [n] with
// fixation map F [n]:
//   1. min / max of S and N = #{F > 0};                                    N == 0, max == min or a NaN in S -> score NaN
//   2. the normalised values (S - min) / (max - min) at F > 0, computed IN THE DTYPE OF S (fp32 for a float map, fp64 once
//      jitter noise was added: the rounding of this step creates ties, and ties change the counts), compacted in any order;
//   3. bitonic sort, descending: t_0 >= ... >= t_{N-1}, padded with -inf to a power of two;
//   4. every pixel finds k = #{ i : t_i > S_p } by binary search and counts hist[k] += 1, k in [0, N];
//   5. inclusive scan: above_i = sum_{k <= i} hist[k] = #{ p : S_p >= t_i };
//   6. trapezoid over tp = [0, 1/N, ..., N/N, 1], fp = [0, ..., (above_i - i - fp_offset) / (n - N), ..., 1] in fp64.
// Steps 2-5 are integers and comparisons of identically rounded values: the counts are exact and do not depend on the order
// of the atomic adds.  Step 6 sums per-lane strided partial sums through the fixed block tree: two runs are bit-identical.
//
// Where the list lives.  A group has 49 KB of static LDS: the sorted list as fp64 (AUC_LDS_CAP x 8 B = 32 KB, one element
// size for both map dtypes) and the histogram ((AUC_LDS_CAP + 1) x 4 B = 16 KB).  With 160 KB per CU that keeps two
// 1024-lane groups resident, which is the CU's wave limit anyway; the next power of two (8192) would need 96 KB and halve
// that.  Maps with more than AUC_LDS_CAP = 4096 fixations (a 1080p DIEM frame can carry 20 000) run the same network and
// the same histogram over the caller's workspace: list [pad2(n)] fp64 + hist [n + 1] int32 per map.  The option "auc_ws"
// sends every map there (tests compare the two routes bit for bit).
//
// Almost every pixel of a real map lies below every threshold (bin N), and the pixels at the maximum land in bin 0: those
// two bins are counted in registers and reduced once per wave, the rest goes through integer atomics.
#include "common.h"

#include <type_traits>

#define AUC_LANES 1024
#define AUC_LDS_CAP 4096

// exclusive prefix (lane order) of one int per lane over the group; *total = the group's sum
VN_DEV int block_excl_scan_i(int v, int* shi, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) shi[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < nw; ++k) {
    if (k < wv) base += shi[k];
    tot += shi[k];
  }
  *total = tot;
  return base + inc - v;
}

// A map's statistics, the first pass of AUC-Judd and of the prep kernel, from what each lane found on its own walk over the pixels
// (min, max, #{F > 0}, a NaN seen; none depends on the walk): lo = min and range = max - min rounded to TS, the dtype the
// normalisation runs in (auc_norm), the fixation count and the NaN flag.  The NaN rule on top of them is each kernel's own.
template <typename TS> struct MapStats { TS lo, range; int N, nbad; };
template <typename TS> VN_DEV MapStats<TS> map_stats(double mn, double mx, int cnt, int bad, double* sh, int* shi) {
  mx = block_max_d(mx, sh);
  mn = -block_max_d(-mn, sh);
  int N, nbad;
  block_excl_scan_i(cnt, shi, &N);
  block_excl_scan_i(bad, shi, &nbad);
  return {(TS)mn, (TS)mx - (TS)mn, N, nbad};
}

// f(TS(), std::bool_constant<F64>()): the kernels' template arguments from the ABI's two dtype flags (saliency map, fixation map)
template <typename F> static void by_dtypes(int s_is_f64, int fix_is_f64, F f) {
  if (s_is_f64) { if (fix_is_f64) f(double(), std::true_type()); else f(double(), std::false_type()); }
  else { if (fix_is_f64) f(float(), std::true_type()); else f(float(), std::false_type()); }
}

// (S_p - min) / (max - min) in the dtype of S: one IEEE subtract and one IEEE divide per element (-ffp-contract=off, fp32
// division correctly rounded), as numpy does it
template <typename TS> VN_DEV double auc_norm(TS v, TS lo, TS range) { return (double)((v - lo) / range); }

// steps 2-6 on a list / histogram that live in LDS or in the workspace (inlined once per address space)
template <typename TS, bool F64>
VN_DEV void auc_rank(const TS* __restrict__ sp, const void* fix, long fb, int n, int N, int npad, TS lo, TS range, int fp_offset,
                     double* lp, int* hp, int* fill, double* sh, int* shi, double* score, int* above) {
  const int tid = threadIdx.x;
  if (tid == 0) *fill = 0;
  for (int i = N + tid; i < npad; i += AUC_LANES) lp[i] = -INFINITY;
  for (int i = tid; i <= N; i += AUC_LANES) hp[i] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += AUC_LANES)
    if (ldg<F64>(fix, fb + i) > 0.0) {
      const int p = atomicAdd(fill, 1);
      if (p < N) lp[p] = auc_norm<TS>(sp[i], lo, range);
    }
  __syncthreads();
  // bitonic network, descending; ties are left where they are (equal values: any order is the same list)
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += AUC_LANES) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const double a = lp[i], c = lp[p];
        if ((i & k) == 0 ? a < c : a > c) { lp[i] = c; lp[p] = a; }
      }
      __syncthreads();
    }
  const double tmax = lp[0], tmin = lp[N - 1];
  int c0 = 0, cN = 0;
  for (int i = tid; i < n; i += AUC_LANES) {
    const double v = auc_norm<TS>(sp[i], lo, range);
    if (tmin > v) ++cN;                       // below every threshold
    else if (!(tmax > v)) ++c0;               // at or above the largest one
    else {                                    // t_0 > v >= t_{N-1}: k in [1, N-1]
      int a = 1, e = N - 1;
      while (a < e) {
        const int mid = (a + e) >> 1;
        if (lp[mid] > v) a = mid + 1; else e = mid;
      }
      atomicAdd(hp + a, 1);
    }
  }
  c0 = wave_sum_i(c0); cN = wave_sum_i(cN);
  if ((tid & 63) == 0) {
    if (c0) atomicAdd(hp, c0);
    if (cN) atomicAdd(hp + N, cN);
  }
  __syncthreads();
  // inclusive scan of hist[0..N-1] in place: a contiguous chunk per lane, the chunk sums scanned over the group
  const int chunk = (N + AUC_LANES - 1) / AUC_LANES;
  const int i0 = tid * chunk < N ? tid * chunk : N, i1 = i0 + chunk < N ? i0 + chunk : N;
  int mine = 0, total;
  for (int i = i0; i < i1; ++i) mine += hp[i];
  int run = block_excl_scan_i(mine, shi, &total);
  for (int i = i0; i < i1; ++i) { run += hp[i]; hp[i] = run; }
  __syncthreads();
  if (above)
    for (int i = tid; i < N; i += AUC_LANES) above[i] = hp[i];
  // np.trapz(tp, x=fp) = sum_j (fp[j+1] - fp[j]) * (tp[j+1] + tp[j]) / 2 over the N + 1 intervals
  const double dN = (double)N, dF = (double)(n - N);
  double acc = 0.0;
  for (int j = tid; j <= N; j += AUC_LANES) {
    const double fp0 = j == 0 ? 0.0 : (double)(hp[j - 1] - (j - 1) - fp_offset) / dF, tp0 = (double)j / dN;
    const double fp1 = j == N ? 1.0 : (double)(hp[j] - j - fp_offset) / dF, tp1 = j == N ? 1.0 : (double)(j + 1) / dN;
    acc += (fp1 - fp0) * (tp1 + tp0) / 2.0;
  }
  acc = block_sum_d(acc, sh);
  if (tid == 0) *score = acc;
}

template <typename TS, bool F64>
__global__ __launch_bounds__(AUC_LANES) void auc_judd_kernel(const TS* __restrict__ s, const void* fix, int n, int fp_offset, int force_ws,
                                                             char* ws, size_t ws_per_map, size_t ws_hist_off, double* __restrict__ score,
                                                             int* __restrict__ nfix, int* above) {
  __shared__ double lst[AUC_LDS_CAP];
  __shared__ int hst[AUC_LDS_CAP + 1];
  __shared__ double sh[16];
  __shared__ int shi[16];
  __shared__ int fill;
  const int b = blockIdx.x, tid = threadIdx.x;
  const TS* sp = s + (long)b * n;
  const long fb = (long)b * n;
  double mn = INFINITY, mx = -INFINITY;
  int cnt = 0, bad = 0;
  for (int i = tid; i < n; i += AUC_LANES) {
    const double v = (double)sp[i];
    mn = fmin(mn, v); mx = fmax(mx, v);
    bad |= v != v;
    cnt += ldg<F64>(fix, fb + i) > 0.0;
  }
  const MapStats<TS> st = map_stats<TS>(mn, mx, cnt, bad, sh, shi);
  const int N = st.N;
  const TS lo = st.lo, range = st.range;
  // loss.py:143-146 (no fixation) and :166-169 (max == min: the normalised map is all NaN; a NaN in S makes min NaN, the same)
  if (N == 0 || st.nbad || !(range > (TS)0)) {
    if (tid == 0) { score[b] = NAN; nfix[b] = N; }
    return;
  }
  if (tid == 0) nfix[b] = N;
  int npad = 1;
  while (npad < N) npad <<= 1;
  int* ab = above ? above + (long)b * n : nullptr;
  if (!force_ws && npad <= AUC_LDS_CAP)
    auc_rank<TS, F64>(sp, fix, fb, n, N, npad, lo, range, fp_offset, lst, hst, &fill, sh, shi, score + b, ab);
  else
    auc_rank<TS, F64>(sp, fix, fb, n, N, npad, lo, range, fp_offset, (double*)(ws + (size_t)b * ws_per_map),
                      (int*)(ws + (size_t)b * ws_per_map + ws_hist_off), &fill, sh, shi, score + b, ab);
}

static size_t auc_pad2(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}
static size_t auc_hist_off(int32_t n) { return auc_pad2((size_t)n) * sizeof(double); }
static size_t auc_ws_per_map(int32_t n) { return auc_hist_off(n) + vn_pad8(((size_t)n + 1) * sizeof(int32_t)); }

extern "C" size_t vinet_auc_judd_workspace(int32_t B, int32_t n) {
  if (B <= 0 || n <= 0) return 0;
  return (size_t)B * auc_ws_per_map(n);
}

extern "C" int vinet_auc_judd(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, int32_t B, int32_t n,
                              int32_t fp_offset, void* workspace, size_t workspace_bytes, double* score, int32_t* nfix,
                              int32_t* above, void* stream) {
  VN_CHECK_ARG(s && fix && score && nfix, "auc_judd: null map, fixation map, score or nfix");
  VN_CHECK_ARG(B > 0 && n > 0 && n <= (1 << 30), "auc_judd: B and n must be positive (n <= 2^30)");
  VN_CHECK_ARG(fp_offset == 0 || fp_offset == 1, "auc_judd: fp_offset is 0 (loss.py) or 1 (AUC_Judd.m)");
  VN_CHECK_ARG(workspace && workspace_bytes >= vinet_auc_judd_workspace(B, n) && (((uintptr_t)workspace) & 7) == 0,
               "auc_judd: workspace of %zu bytes (8-byte aligned) needed, got %zu", vinet_auc_judd_workspace(B, n), workspace ? workspace_bytes : (size_t)0);
  hipStream_t st = (hipStream_t)stream;
  const size_t per = auc_ws_per_map(n), hoff = auc_hist_off(n);
  const int fw = g_vinet_opt_auc_ws;
  by_dtypes(s_is_f64, fix_is_f64, [&](auto ts, auto f64) {
    using TS = decltype(ts);
    hipLaunchKernelGGL((auc_judd_kernel<TS, decltype(f64)::value>), dim3(B), dim3(AUC_LANES), 0, st, (const TS*)s, fix, n, fp_offset, fw,
                       (char*)workspace, per, hoff, score, nfix, above);
  });
  return vn_launch_status("auc_judd");
}

// ---- shuffled AUC (code_for_Metrics/AUC_shuffled.m, createShuffmap1.m, eval_diem.m:65) and AUC-Borji (AUC_Borji.m) ----------------
//
// Per map: N fixations, the other set { p : O_p > 0 and not F_p > 0 } of size M, K = min(N, M), thresholds t_k = k * step
// (fp64, k = 0 .. T-1: every k with t_k <= 1).  A normalised value v falls in bin j(v) = #{ k : t_k <= v } in [1, T], found by
// binary search with the comparison `k * step <= v` itself (never floor(v / step): the two differ where v sits on a threshold).
// #{ v >= t_k } = #{ j(v) >= k + 1 } is a suffix sum of the bin counts: integers, exact in any order.  Three launches:
//   sauc_prep_kernel   one workgroup per map: min / max / N / M, the suffix counts of the fixations (the tp side, the same for
//                      every split) and the other set as a list of pixel indices in ascending order, into the workspace;
//   split_auc_kernel   grid (map, split group): per split the K locations (given, or drawn: below), their bin counts, the
//                      suffix sum and the trapezoid area through the fixed block tree, into the workspace;
//   sauc_mean_kernel   one lane per map: the mean of the areas in split order.
// The (map, split) pairs are independent and every sum has a fixed order, so the number of split groups (chosen from B to fill
// the chip) changes no bit.  AUC-Borji is the same three launches with another draw (BorjiDraw, below) and no other set.
//
// The shuffled draw (ShuffledDraw).  Location p of split j has the key h = mix32(mix32(p ^ k0) + k1), (k0, k1) from (seed, frame id, j): a bijection of
// p, so the keys of a map's locations are distinct and "the K smallest keys" is a set of exactly K.  The K-th smallest key is
// found by a radix select over the list, 11 + 11 + 10 bits with a 2048-bin LDS histogram (three passes that recompute the keys:
// no key list, no sort), and a fourth pass bins the locations whose key is <= it.  K == M takes the whole list.
//
// LDS of the split kernel: two count arrays (SAUC_MAX_T + 1) x 4 B = 8 KB each and, with the shuffled draw only, the list
// 8192 x 4 B = 32 KB and the radix histogram 8 KB: 56 KB, under the 64 KB a static allocation may take (two groups would fit a CU; the kernel's 80 VGPRs allow one).  A DIEM
// video's union map has 10^4 .. 10^5 locations: those lists are read from the workspace (L2-resident, coalesced) by the same code.
#define SAUC_LDS_CAP 8192
#define SAUC_MAX_T 2048
#define SAUC_RADIX 2048

struct SaucHead { double lo, range; int32_t N, M, nan, pad; };

VN_DEV bool sauc_other_on(const void* o, int kind, long i) {
  if (kind == 0) return ((const uint8_t*)o)[i] > 0;
  if (kind == 1) return ((const float*)o)[i] > 0.f;
  return ((const double*)o)[i] > 0.0;
}
// #{ k in [0, T) : k * step <= v }
VN_DEV int sauc_bin(double v, double step, int T) {
  int a = 0, e = T;
  while (a < e) {
    const int mid = (a + e) >> 1;
    if ((double)mid * step <= v) a = mid + 1; else e = mid;
  }
  return a;
}
// h[j] += 1 for every active lane; whole waves call it.  With few bins (step 0.1 has 12) most lanes hit the same one: a ballot
// per bin and one atomic per wave instead of 64 serialised ones.
VN_DEV void sauc_count(int* h, int j, bool active, int nb) {
  if (nb <= 16) {
    for (int q = 0; q < nb; ++q) {
      const unsigned long long m = __ballot(active && j == q);
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(h + q, __popcll(m));
    }
  } else if (active) {
    atomicAdd(h + j, 1);
  }
}
// h[j] <- sum_{i >= j} h[i], j in [0, nb), in place: a contiguous chunk per lane from the top, the chunk sums scanned over the group
VN_DEV void sauc_suffix(int* h, int nb, int* shi) {
  __syncthreads();
  const int tid = threadIdx.x, chunk = (nb + AUC_LANES - 1) / AUC_LANES;
  const int r0 = tid * chunk < nb ? tid * chunk : nb, r1 = r0 + chunk < nb ? r0 + chunk : nb;
  int mine = 0, total;
  for (int r = r0; r < r1; ++r) mine += h[nb - 1 - r];
  int run = block_excl_scan_i(mine, shi, &total);
  for (int r = r0; r < r1; ++r) { run += h[nb - 1 - r]; h[nb - 1 - r] = run; }
  __syncthreads();
}
VN_DEV void sauc_keys(int64_t seed, int64_t frame, int split, uint32_t* k0, uint32_t* k1) {
  uint32_t x = mix32((uint32_t)seed ^ 0x9e3779b9u);
  x = mix32(x + (uint32_t)((uint64_t)seed >> 32));
  x = mix32(x ^ (uint32_t)frame);
  x = mix32(x + (uint32_t)((uint64_t)frame >> 32));
  *k0 = mix32(x ^ ((uint32_t)split * 0x85ebca6bu));
  *k1 = mix32(*k0 + 0x9e3779b9u) ^ x;
}
VN_DEV uint32_t sauc_key(uint32_t p, uint32_t k0, uint32_t k1) { return mix32(mix32(p ^ k0) + k1); }

// `oth` == nullptr (AUC-Borji, below): there is no other set, M = n and no list.  `min_fix`: fewer fixations than that give NaN
// (1 for the shuffled AUC, 2 for AUC-Borji).
template <typename TS, bool F64>
__global__ __launch_bounds__(AUC_LANES) void sauc_prep_kernel(const TS* __restrict__ s, const void* fix, const void* oth, int okind, long ostride,
                                                              int n, int min_fix, double step, int T, int want_list, char* ws,
                                                              size_t ws_per_map, size_t ws_list_off) {
  __shared__ int hst[SAUC_MAX_T + 1];
  __shared__ double sh[16];
  __shared__ int shi[16];
  __shared__ int wcnt[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const TS* sp = s + (long)b * n;
  const long fb = (long)b * n, ob = (long)b * ostride;
  char* wm = ws + (size_t)b * ws_per_map;
  SaucHead* head = (SaucHead*)wm;
  int* tpc = (int*)(wm + sizeof(SaucHead));
  int* list = (int*)(wm + ws_list_off);
  // each wave walks one contiguous segment in steps of 64: the list below comes out in pixel order without a sort
  const int seg = (int)(((long)n + AUC_LANES - 1) / AUC_LANES) * 64;
  const long i0 = (long)wv * seg, i1 = i0 + seg < n ? i0 + seg : n;
  double mn = INFINITY, mx = -INFINITY;
  int cnt = 0, bad = 0, co = 0;
  for (long i = i0 + lane; i < i1; i += 64) {
    const double v = (double)sp[i];
    mn = fmin(mn, v); mx = fmax(mx, v);
    bad |= v != v;
    const bool f = ldg<F64>(fix, fb + i) > 0.0;
    cnt += f;
    co += oth && !f && sauc_other_on(oth, okind, ob + i);
  }
  const MapStats<TS> st = map_stats<TS>(mn, mx, cnt, bad, sh, shi);
  const int N = st.N;
  co = wave_sum_i(co);
  if (lane == 0) wcnt[wv] = co;
  __syncthreads();
  int M = 0, base = 0;
  for (int k = 0; k < AUC_LANES / 64; ++k) {
    if (k < wv) base += wcnt[k];
    M += wcnt[k];
  }
  if (!oth) M = n;
  const TS lo = st.lo, range = st.range;
  // AUC_shuffled.m:33-36 (no fixation; AUC_Borji.m:31 with <= 1), :46-49 (constant map / NaN), and 0/0 of an empty other set
  const int nan = N < min_fix || st.nbad || !(range > (TS)0) || M == 0;
  if (tid == 0) { head->lo = (double)lo; head->range = (double)range; head->N = N; head->M = M; head->nan = nan; head->pad = 0; }
  if (nan) return;
  for (int i = tid; i <= T; i += AUC_LANES) hst[i] = 0;
  __syncthreads();
  for (long c = i0; c < i1; c += 64) {
    const long i = c + lane;
    const bool f = i < i1 && ldg<F64>(fix, fb + i) > 0.0;
    const int j = f ? sauc_bin(auc_norm<TS>(sp[i], lo, range), step, T) : 0;
    sauc_count(hst, j, f, T + 1);
    if (want_list) {
      const bool o = i < i1 && !f && sauc_other_on(oth, okind, ob + i);
      const unsigned long long m = __ballot(o);
      if (o) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (int)i;
      base += __popcll(m);
    }
  }
  sauc_suffix(hst, T + 1, shi);
  for (int i = tid; i <= T; i += AUC_LANES) tpc[i] = hst[i];
}

// what the split stage needs to bin a pixel of its map
template <typename TS> struct SaucMap {
  const TS* sp; int n; TS lo, range; double step; int T;
  VN_DEV int bin(int p) const { return sauc_bin(auc_norm<TS>(sp[p], lo, range), step, T); }
};

// one split's locations as the caller gave them (a row of `samples`: pixel indices, then -1): their bin counts into cnt, the number
// of valid ones into *fill.  Every lane of the group calls it; cnt and *fill were zeroed by the caller.
template <typename TS> VN_DEV void sauc_given(const SaucMap<TS>& m, const int32_t* row, int kmax, int* cnt, int* fill) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int c = 0; c < kmax; c += AUC_LANES) {
    const int p = c + tid < kmax ? row[c + tid] : -1;
    const bool act = p >= 0 && p < m.n;
    const int j = act ? m.bin(p) : 0;
    sauc_count(cnt, j, act, m.T + 1);
    const unsigned long long msk = __ballot(act);
    if ((tid & 63) == 0 && msk) atomicAdd(fill, __popcll(msk));
  }
}
// the area of one split from the suffix counts cnt (the locations, K of them) and tpc (the fixations, N of them):
// points P_0 = (0,0), P_i = (fp_k, tp_k) with k = T - i for i = 1 .. T, P_{T+1} = (1,1); trapz over the T + 1 intervals
VN_DEV double sauc_trapz(const int* cnt, const int* tpc, int T, double dK, double dN, double* sh) {
  double acc = 0.0;
  for (int i = threadIdx.x; i <= T; i += AUC_LANES) {
    const double x0 = i == 0 ? 0.0 : (double)cnt[T - i + 1] / dK, y0 = i == 0 ? 0.0 : (double)tpc[T - i + 1] / dN;
    const double x1 = i == T ? 1.0 : (double)cnt[T - i] / dK, y1 = i == T ? 1.0 : (double)tpc[T - i] / dN;
    acc += (x1 - x0) * (y1 + y0) / 2.0;
  }
  return block_sum_d(acc, sh);
}

// ---- the two draws of split_auc_kernel: set up once per workgroup (`with`: every lane calls it, and it calls the split loop with the
// draw), a draw says how many locations a split takes (`K`) and, per split, counts the bins of its K locations into cnt, leaves their
// number in *fill and writes them to `out` (if not null, at most kmax).  `draw` is entered with cnt and *fill zeroed by lanes that
// have not met a barrier since: its first barrier comes before it counts.  (k0, k1) = sauc_keys(seed ^ DOMAIN, frame id, split).

// The shuffled AUC: the K = min(N, M) locations with the smallest keys among the M of the other set (no repeats, no fixation).
// Owns the list and where it is read from: a copy in LDS, or the workspace for M > SAUC_LDS_CAP, given samples (prep wrote no list
// then) and the option "sauc_ws"; the split loop is inlined once per address space.
struct ShuffledDraw {
  static constexpr int64_t DOMAIN = 0;
  const int* lp;           // the other set, ascending pixel indices
  int M;
  int* rad;                // radix histogram
  int* sel;                // the digit a pass selected, the rank left within it

  template <typename F> VN_DEV static void with(int M, const int* list, bool given, int force_ws, F splits) {
    __shared__ int lst[SAUC_LDS_CAP];
    __shared__ int rad[SAUC_RADIX];
    __shared__ int sel[2];
    const bool in_lds = !given && !force_ws && M <= SAUC_LDS_CAP;
    if (in_lds)
      for (int i = threadIdx.x; i < M; i += AUC_LANES) lst[i] = list[i];
    __syncthreads();
    if (in_lds) splits(ShuffledDraw{lst, M, rad, sel});
    else splits(ShuffledDraw{list, M, rad, sel});
  }
  VN_DEV int K(int N) const { return N < M ? N : M; }

  template <typename TS>
  VN_DEV void draw(const SaucMap<TS>& m, int K, uint32_t k0, uint32_t k1, int* cnt, int* fill, int* shi, int32_t* out, int kmax) const {
    const int tid = threadIdx.x;
    uint32_t kth = 0xffffffffu;
    if (K < M) {
      // radix select of the K-th smallest key: digits of 11, 11 and 10 bits
      uint32_t prefix = 0;
      int need = K;
      for (int pass = 0; pass < 3; ++pass) {
        const int bits = pass == 2 ? 10 : 11, shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, nbin = 1 << bits;
        for (int i = tid; i < nbin; i += AUC_LANES) rad[i] = 0;
        __syncthreads();
        for (int i = tid; i < M; i += AUC_LANES) {
          const uint32_t h = sauc_key((uint32_t)lp[i], k0, k1);
          if (pass == 0 || (h >> (shift + bits)) == prefix) atomicAdd(rad + ((h >> shift) & (uint32_t)(nbin - 1)), 1);
        }
        __syncthreads();
        const int c0 = 2 * tid < nbin ? rad[2 * tid] : 0, c1 = 2 * tid < nbin ? rad[2 * tid + 1] : 0;
        int total;
        const int ex = block_excl_scan_i(c0 + c1, shi, &total);
        if (ex < need && need <= ex + c0) { sel[0] = 2 * tid; sel[1] = need - ex; }
        else if (ex + c0 < need && need <= ex + c0 + c1) { sel[0] = 2 * tid + 1; sel[1] = need - ex - c0; }
        __syncthreads();
        prefix = (prefix << bits) | (uint32_t)sel[0];
        need = sel[1];
        __syncthreads();
      }
      kth = prefix;
    } else {
      __syncthreads();
    }
    for (int c = 0; c < M; c += AUC_LANES) {
      const int i = c + tid;
      const int p = i < M ? lp[i] : 0;
      const bool act = i < M && sauc_key((uint32_t)p, k0, k1) <= kth;
      const int j = act ? m.bin(p) : 0;
      sauc_count(cnt, j, act, m.T + 1);
      const unsigned long long msk = __ballot(act);
      int slot = 0;
      if ((tid & 63) == 0 && msk) slot = atomicAdd(fill, __popcll(msk));
      slot = __shfl(slot, 0, 64) + __popcll(msk & ((1ull << (tid & 63)) - 1ull));
      if (out && act && slot < kmax) out[slot] = p;
    }
  }
};

// AUC-Borji (code_for_Metrics/AUC_Borji.m): the shuffled AUC with another draw of the negative locations: K = N of them per split,
// uniform over ALL n pixels, with replacement (AUC_Borji.m:58 `randi([1 Npixels], [Nfixations, Nsplits])`): a fixation pixel may be
// drawn and a pixel may repeat.  tp and fp are both divided by N (:75-76), one fixation or none is NaN (:31: sauc_prep_kernel's
// min_fix = 2).  The sweep `0:stepSize:max([Sth;curfix])` of :67 is the shuffled AUC's "every t_k <= 1" for the same reason: a
// threshold above every value gives the point (0, 0) again, zero area.  There is no list and no select: sample j of a split is pixel
// ((uint64)h * n) >> 32 with h = sauc_key(j, k0, k1) -- a function of (seed, frame id, split, j) alone, and (DOMAIN) not the stream
// the shuffled AUC draws from under the same seed.
struct BorjiDraw {
  static constexpr int64_t DOMAIN = 0x426f726a69415543ll;          // "BorjiAUC"

  template <typename F> VN_DEV static void with(int, const int*, bool, int, F splits) { splits(BorjiDraw{}); }
  VN_DEV int K(int N) const { return N; }

  template <typename TS>
  VN_DEV void draw(const SaucMap<TS>& m, int K, uint32_t k0, uint32_t k1, int* cnt, int* fill, int*, int32_t* out, int kmax) const {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int c = 0; c < K; c += AUC_LANES) {
      const int j = c + tid;
      const bool act = j < K;
      const int p = act ? (int)(((uint64_t)sauc_key((uint32_t)j, k0, k1) * (uint64_t)(uint32_t)m.n) >> 32) : 0;      // in [0, n)
      const int bin = act ? m.bin(p) : 0;
      sauc_count(cnt, bin, act, m.T + 1);
      if (out && act && j < kmax) out[j] = p;
    }
    if (tid == 0) *fill = K;
  }
};

// grid (map, split group): the splits g, g + G, ... of one map, each from the caller's samples or from Draw
template <typename TS, typename Draw>
__global__ __launch_bounds__(AUC_LANES) void split_auc_kernel(const TS* __restrict__ s, int n, int nsplits, double step, int T, int64_t seed,
                                                              const int64_t* frame_ids, const int32_t* samples, int kmax, int force_ws,
                                                              char* ws, size_t ws_map0, size_t ws_per_map, size_t ws_list_off,
                                                              int32_t* samples_out) {
  __shared__ int tpc[SAUC_MAX_T + 1];
  __shared__ int cnt[SAUC_MAX_T + 1];
  __shared__ double sh[16];
  __shared__ int shi[16];
  __shared__ int fill;
  const int b = blockIdx.x, tid = threadIdx.x;
  const char* wm = ws + ws_map0 + (size_t)b * ws_per_map;
  const SaucHead* head = (const SaucHead*)wm;
  int32_t* outb = samples_out ? samples_out + (long)b * nsplits * kmax : nullptr;
  if (head->nan) {                               // sauc_mean_kernel writes the NaN; the sample rows of such a map are empty
    if (outb)
      for (int sp_i = blockIdx.y; sp_i < nsplits; sp_i += gridDim.y)
        for (int i = tid; i < kmax; i += AUC_LANES) outb[(long)sp_i * kmax + i] = -1;
    return;
  }
  const int N = head->N, M = head->M;
  const SaucMap<TS> m = {s + (long)b * n, n, (TS)head->lo, (TS)head->range, step, T};
  const int* tp_ws = (const int*)(wm + sizeof(SaucHead));
  for (int i = tid; i <= T; i += AUC_LANES) tpc[i] = tp_ws[i];
  const int64_t frame = frame_ids ? frame_ids[b] : (int64_t)b;
  const int32_t* smp = samples ? samples + (long)b * nsplits * kmax : nullptr;
  double* auc = (double*)ws + (long)b * nsplits;
  Draw::with(M, (const int*)(wm + ws_list_off), samples != nullptr, force_ws, [&](const Draw& draw) __attribute__((always_inline)) {
    const int K = draw.K(N);
    const double dN = (double)N, dK = (double)K;
    for (int sp_i = blockIdx.y; sp_i < nsplits; sp_i += gridDim.y) {
      for (int i = tid; i <= T; i += AUC_LANES) cnt[i] = 0;
      if (tid == 0) fill = 0;
      int32_t* out = outb ? outb + (long)sp_i * kmax : nullptr;
      if (smp) {                                  // (either way a barrier comes before the first count: cnt and fill are zero then)
        sauc_given<TS>(m, smp + (long)sp_i * kmax, kmax, cnt, &fill);
      } else {
        uint32_t k0, k1;
        sauc_keys(seed ^ Draw::DOMAIN, frame, sp_i, &k0, &k1);
        draw.template draw<TS>(m, K, k0, k1, cnt, &fill, shi, out, kmax);
      }
      sauc_suffix(cnt, T + 1, shi);                 // cnt[j] = #{ curfix in bin >= j }; fill = the locations counted
      const int got = fill;
      if (out && !smp)
        for (int i = got + tid; i < kmax; i += AUC_LANES) out[i] = -1;
      const double acc = sauc_trapz(cnt, tpc, T, dK, dN, sh);
      if (tid == 0) auc[sp_i] = got == K ? acc : NAN;
    }
  });
}

__global__ void sauc_mean_kernel(const char* ws, size_t ws_map0, size_t ws_per_map, int B, int nsplits, double* __restrict__ score,
                                 int* __restrict__ nfix, int* __restrict__ nother) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const SaucHead* head = (const SaucHead*)(ws + ws_map0 + (size_t)b * ws_per_map);
  nfix[b] = head->N;
  if (nother) nother[b] = head->M;
  if (head->nan) { score[b] = NAN; return; }
  const double* auc = (const double*)ws + (long)b * nsplits;
  double acc = 0.0;
  for (int i = 0; i < nsplits; ++i) acc += auc[i];
  score[b] = acc / (double)nsplits;
}

// the number of k = 0, 1, ... with k * step <= 1 (0: more than SAUC_MAX_T, or no valid step)
static int sauc_thresholds(double step) {
  if (!(step > 0.0 && step <= 1.0) || 1.0 / step > (double)(SAUC_MAX_T - 1)) return 0;
  int T = (int)(1.0 / step) + 1;
  while ((double)T * step <= 1.0) ++T;
  while (T > 1 && (double)(T - 1) * step > 1.0) --T;
  return T <= SAUC_MAX_T ? T : 0;
}
static size_t sauc_list_off(int T) { return sizeof(SaucHead) + vn_pad8(((size_t)T + 1) * sizeof(int32_t)); }
static size_t sauc_ws_per_map(int32_t n, int T) { return sauc_list_off(T) + vn_pad8((size_t)n * sizeof(int32_t)); }
// the areas [B][nsplits] fp64, then a section per map; without a list (AUC-Borji) it ends where the list would begin
static size_t split_workspace(int32_t B, int32_t n, int32_t nsplits, double step, bool with_list) {
  const int T = sauc_thresholds(step);
  if (B <= 0 || n <= 0 || n > (1 << 30) || nsplits <= 0 || T == 0) return 0;
  return (size_t)B * nsplits * sizeof(double) + (size_t)B * (with_list ? sauc_ws_per_map(n, T) : sauc_list_off(T));
}

// the arguments the two split metrics share (`who`: the entry point, for the message); *T = the number of thresholds
static int split_check(const char* who, int32_t B, int32_t n, int32_t nsplits, double step, const int32_t* samples,
                       const int32_t* samples_out, int32_t kmax, const void* workspace, size_t workspace_bytes, size_t need, int* T) {
  VN_CHECK_ARG(B > 0 && n > 0 && n <= (1 << 30) && nsplits > 0, "%s: B, n and nsplits must be positive (n <= 2^30)", who);
  VN_CHECK_ARG(step > 0.0 && step <= 1.0, "%s: step must lie in (0, 1]", who);
  *T = sauc_thresholds(step);
  VN_CHECK_ARG(*T > 0, "%s: step %g gives more than %d thresholds", who, step, SAUC_MAX_T);
  VN_CHECK_ARG((!samples && !samples_out) || kmax > 0, "%s: kmax must be positive with samples or samples_out", who);
  VN_CHECK_ARG(!(samples && samples_out), "%s: samples_out returns the device draw; the given samples are the caller's already", who);
  VN_CHECK_ARG(workspace && workspace_bytes >= need && (((uintptr_t)workspace) & 7) == 0,
               "%s: workspace of %zu bytes (8-byte aligned) needed, got %zu", who, need, workspace ? workspace_bytes : (size_t)0);
  return 0;
}
// split groups per map: enough workgroups for the chip's 256 CUs x 2 whatever B is; the result does not depend on it
static int split_groups(int B, int nsplits) {
  int G = 2048 / B;
  G = G < 1 ? 1 : (G > 32 ? 32 : G);
  return G > nsplits ? nsplits : G;
}
// the three launches of a split metric on a checked call.  `other` == nullptr: no other set (AUC-Borji)
template <typename Draw>
static void split_auc_launch(const void* s, int s_is_f64, const void* fix, int fix_is_f64, const void* other, int other_kind, long other_stride,
                             int B, int n, int min_fix, int nsplits, double step, int T, int64_t seed, const int64_t* frame_ids,
                             const int32_t* samples, int kmax, int force_ws, char* ws, size_t per, size_t loff, double* score, int32_t* nfix,
                             int32_t* nother, int32_t* samples_out, hipStream_t st) {
  const size_t map0 = (size_t)B * nsplits * sizeof(double);
  const int G = split_groups(B, nsplits), want_list = other && !samples;
  by_dtypes(s_is_f64, fix_is_f64, [&](auto ts, auto f64) {
    using TS = decltype(ts);
    hipLaunchKernelGGL((sauc_prep_kernel<TS, decltype(f64)::value>), dim3(B), dim3(AUC_LANES), 0, st, (const TS*)s, fix, other, other_kind,
                       other_stride, n, min_fix, step, T, want_list, ws + map0, per, loff);
    hipLaunchKernelGGL((split_auc_kernel<TS, Draw>), dim3(B, G), dim3(AUC_LANES), 0, st, (const TS*)s, n, nsplits, step, T, seed, frame_ids,
                       samples, kmax, force_ws, ws, map0, per, loff, samples_out);
  });
  hipLaunchKernelGGL(sauc_mean_kernel, dim3((B + 63) / 64), dim3(64), 0, st, ws, map0, per, B, nsplits, score, nfix, nother);
}

extern "C" size_t vinet_auc_shuffled_workspace(int32_t B, int32_t n, int32_t nsplits, double step) {
  return split_workspace(B, n, nsplits, step, true);
}

extern "C" int vinet_auc_shuffled(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, const void* other,
                                  int32_t other_kind, int64_t other_stride, int32_t B, int32_t n, int32_t nsplits, double step,
                                  int64_t seed, const int64_t* frame_ids, const int32_t* samples, int32_t kmax, void* workspace,
                                  size_t workspace_bytes, double* score, int32_t* nfix, int32_t* nother, int32_t* samples_out,
                                  void* stream) {
  VN_CHECK_ARG(s && fix && other && score && nfix && nother, "auc_shuffled: null map, fixation map, other map, score, nfix or nother");
  VN_CHECK_ARG(other_kind >= 0 && other_kind <= 2, "auc_shuffled: other_kind is 0 (uint8), 1 (fp32) or 2 (fp64)");
  VN_CHECK_ARG(other_stride == 0 || other_stride >= n, "auc_shuffled: other_stride is 0 (one map for the batch) or >= n");
  int T;
  if (split_check("auc_shuffled", B, n, nsplits, step, samples, samples_out, kmax, workspace, workspace_bytes,
                  vinet_auc_shuffled_workspace(B, n, nsplits, step), &T))
    return -1;
  split_auc_launch<ShuffledDraw>(s, s_is_f64, fix, fix_is_f64, other, other_kind, (long)other_stride, B, n, 1, nsplits, step, T, seed, frame_ids,
                                 samples, kmax, g_vinet_opt_sauc_ws, (char*)workspace, sauc_ws_per_map(n, T), sauc_list_off(T), score, nfix,
                                 nother, samples_out, (hipStream_t)stream);
  return vn_launch_status("auc_shuffled");
}

extern "C" size_t vinet_auc_borji_workspace(int32_t B, int32_t n, int32_t nsplits, double step) {
  return split_workspace(B, n, nsplits, step, false);
}

extern "C" int vinet_auc_borji(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, int32_t B, int32_t n, int32_t nsplits,
                               double step, int64_t seed, const int64_t* frame_ids, const int32_t* samples, int32_t kmax, void* workspace,
                               size_t workspace_bytes, double* score, int32_t* nfix, int32_t* samples_out, void* stream) {
  VN_CHECK_ARG(s && fix && score && nfix, "auc_borji: null map, fixation map, score or nfix");
  int T;
  if (split_check("auc_borji", B, n, nsplits, step, samples, samples_out, kmax, workspace, workspace_bytes,
                  vinet_auc_borji_workspace(B, n, nsplits, step), &T))
    return -1;
  split_auc_launch<BorjiDraw>(s, s_is_f64, fix, fix_is_f64, nullptr, 0, 0l, B, n, 2, nsplits, step, T, seed, frame_ids, samples, kmax, 0,
                              (char*)workspace, sauc_list_off(T), sauc_list_off(T), score, nfix, nullptr, samples_out, (hipStream_t)stream);
  return vn_launch_status("auc_borji");
}

// ---- information gain (code_for_Metrics/InfoGain.m, IG.m) ---------------------------------------------------------------------------
//
// Per map, everything in fp64 on the input values: v = (s - min) / (max - min) (InfoGain.m:17, IG.m:13), p = v / sum(v)
// (InfoGain.m:22, IG.m:17), the same for the baseline map (InfoGain.m:18,23; IG.m:21-23), and
// score = mean over the fixations of log2(eps + p) - log2(eps + pb), eps = 2^-52 (InfoGain.m:27, IG.m:25,35); without a baseline
// the second term is absent (IG.m:28-31).  A fixation is `fix > 0` as everywhere in this library (the .m files take
// logical(fixationMap); fixation maps are non-negative).  One workgroup per map, three passes: min / max / NaN / N, the two sums,
// the fixations; every reduction is per-lane strided partial results through the fixed block tree: two runs agree bit for bit
// and a map's score does not depend on the batch.  NaN: no fixation (the mean of nothing), a constant map or baseline (0/0
// everywhere), a NaN in either.  The first pass keeps its own reduction, the baseline's two maxima between the map's and the counts:
// through map_stats the same loops, with other registers, measured 0.3 ... 0.6 % slower at 360x640 and 1080x1920.
__global__ __launch_bounds__(AUC_LANES) void info_gain_kernel(const void* __restrict__ s, int s64, const void* __restrict__ fix, int f64,
                                                              const void* __restrict__ base, int b64, long bstride, int n,
                                                              double* __restrict__ score, int* __restrict__ nfix) {
  __shared__ double sh[16];
  __shared__ int shi[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long sb = (long)b * n, bb = (long)b * bstride;
  double mn = INFINITY, mx = -INFINITY, mnb = INFINITY, mxb = -INFINITY;
  int cnt = 0, bad = 0;
  for (int i = tid; i < n; i += AUC_LANES) {
    const double v = ldg_rt(s, s64, sb + i);
    mn = fmin(mn, v); mx = fmax(mx, v);
    bad |= v != v;
    cnt += ldg_rt(fix, f64, sb + i) > 0.0;
    if (base) {
      const double w = ldg_rt(base, b64, bb + i);
      mnb = fmin(mnb, w); mxb = fmax(mxb, w);
      bad |= w != w;
    }
  }
  mx = block_max_d(mx, sh);
  mn = -block_max_d(-mn, sh);
  if (base) {
    mxb = block_max_d(mxb, sh);
    mnb = -block_max_d(-mnb, sh);
  }
  int N, nbad;
  block_excl_scan_i(cnt, shi, &N);
  block_excl_scan_i(bad, shi, &nbad);
  const double range = mx - mn, rangeb = mxb - mnb;
  if (tid == 0) nfix[b] = N;
  if (N == 0 || nbad || !(range > 0.0) || (base && !(rangeb > 0.0))) {
    if (tid == 0) score[b] = NAN;
    return;
  }
  double sum = 0.0, sumb = 0.0;
  for (int i = tid; i < n; i += AUC_LANES) {
    sum += (ldg_rt(s, s64, sb + i) - mn) / range;
    if (base) sumb += (ldg_rt(base, b64, bb + i) - mnb) / rangeb;
  }
  sum = block_sum_d(sum, sh);
  if (base) sumb = block_sum_d(sumb, sh);
  const double eps = 2.220446049250313e-16;       // MATLAB's eps = 2^-52
  double acc = 0.0;
  for (int i = tid; i < n; i += AUC_LANES)
    if (ldg_rt(fix, f64, sb + i) > 0.0) {
      double t = log2(eps + (ldg_rt(s, s64, sb + i) - mn) / range / sum);
      if (base) t -= log2(eps + (ldg_rt(base, b64, bb + i) - mnb) / rangeb / sumb);
      acc += t;
    }
  acc = block_sum_d(acc, sh);
  if (tid == 0) score[b] = acc / (double)N;
}

extern "C" int vinet_info_gain(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, const void* baseline,
                               int32_t baseline_is_f64, int64_t baseline_stride, int32_t B, int32_t n, double* score, int32_t* nfix,
                               void* stream) {
  VN_CHECK_ARG(s && fix && score && nfix, "info_gain: null map, fixation map, score or nfix");
  VN_CHECK_ARG(B > 0 && n > 0 && n <= (1 << 30), "info_gain: B and n must be positive (n <= 2^30)");
  VN_CHECK_ARG(baseline_stride == 0 || baseline_stride >= n, "info_gain: baseline_stride is 0 (one map for the batch) or >= n");
  hipLaunchKernelGGL(info_gain_kernel, dim3(B), dim3(AUC_LANES), 0, (hipStream_t)stream, s, s_is_f64 ? 1 : 0, fix, fix_is_f64 ? 1 : 0, baseline,
                     baseline_is_f64 ? 1 : 0, (long)baseline_stride, n, score, nfix);
  return vn_launch_status("info_gain");
}
