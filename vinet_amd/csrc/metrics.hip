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
  mx = block_max_d(mx, sh);
  mn = -block_max_d(-mn, sh);
  int N, nbad;
  block_excl_scan_i(cnt, shi, &N);
  block_excl_scan_i(bad, shi, &nbad);
  const TS lo = (TS)mn, range = (TS)mx - (TS)mn;
  // loss.py:143-146 (no fixation) and :166-169 (max == min: the normalised map is all NaN; a NaN in S makes min NaN, the same)
  if (N == 0 || nbad || !(range > (TS)0)) {
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
static size_t auc_ws_per_map(int32_t n) { return auc_hist_off(n) + (((size_t)n + 1) * sizeof(int32_t) + 7) / 8 * 8; }

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
#define AUC_LAUNCH(TS, F64) \
  hipLaunchKernelGGL((auc_judd_kernel<TS, F64>), dim3(B), dim3(AUC_LANES), 0, st, (const TS*)s, fix, n, fp_offset, fw, (char*)workspace, per, hoff, score, nfix, above)
  if (s_is_f64) { if (fix_is_f64) AUC_LAUNCH(double, true); else AUC_LAUNCH(double, false); }
  else { if (fix_is_f64) AUC_LAUNCH(float, true); else AUC_LAUNCH(float, false); }
#undef AUC_LAUNCH
  return vn_launch_status("auc_judd");
}
