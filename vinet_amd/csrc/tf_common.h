// The stages of transformer.hip that token_encoder.hip reuses, as a header: the counter-based dropout masks, the token GEMM on the
// fp32 MFMA with its epilogues, the LayerNorm pair (templates over the registers per lane and the rows per partial-sum group) and the
// fixed-order reductions of partial gradients.  transformer.hip keeps its own text of them and is built as before; the keep-mask hash,
// the stream numbering and the GEMM epilogues of the two must stay the same text until they are folded into one.
#pragma once
#include "common.h"

namespace {

constexpr int TF_WGRAD_CHUNK = 512;   // tokens per weight-gradient slice (a multiple of 16)

// ---- counter-based keep masks -------------------------------------------------------------------------------------------
// keep(element) = mix(mix(element ^ k0) ^ k1 ^ stream) >= p * 2^32, with (k0, k1) from (seed, step) and stream = 4 layer + site.
// `mix` is the 32-bit finaliser "lowbias32" (public domain).  Sites: 0 attention weights, 1 after the attention projection,
// 2 between the two linears, 3 after the second linear.
struct Drop {
  const int64_t* step;     // device: the step this forward drew (copied into the workspace by tf_step_kernel)
  uint32_t seed_lo, seed_hi, thr;
  float scale;             // 1 / (1 - p)
};
struct DropKey { uint32_t k0, k1, thr; float scale; };
VN_DEV DropKey drop_key(const Drop& d, int stream) {
  DropKey k;
  k.thr = d.thr; k.scale = d.scale; k.k0 = k.k1 = 0;
  if (d.thr) {
    const uint64_t st = (uint64_t)*d.step;
    k.k0 = mix32(d.seed_lo + (uint32_t)st * 0x85ebca6bu);
    k.k1 = mix32((d.seed_hi ^ (uint32_t)(st >> 32)) + k.k0) ^ ((uint32_t)stream * 0x9e3779b9u);
  }
  return k;
}
VN_DEV bool drop_keep(const DropKey& k, uint32_t elem) { return mix32(mix32(elem ^ k.k0) ^ k.k1) >= k.thr; }

__global__ void tf_step_kernel(int64_t* counter, int64_t* drawn) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int64_t s = *counter;
    *drawn = s;
    *counter = s + 1;
  }
}

static inline Drop tf_make_drop(float p, uint64_t seed, const int64_t* drawn) {
  Drop r;
  const bool on = p > 0.f;
  r.step = drawn;
  r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32);
  double t = (double)p * 4294967296.0;
  r.thr = on ? (uint32_t)(t < 1.0 ? 1.0 : (t > 4294967295.0 ? 4294967295.0 : t)) : 0u;
  r.scale = on ? 1.f / (1.f - p) : 1.f;
  return r;
}

// ---- token GEMM on the fp32 MFMA ------------------------------------------------------------------------------------------
// C[M][N] = sum_k A(m,k) B(k,n) with epilogue.  AK: A(m,k) = A[m lda + k] (true) or A[k lda + m];  BK: B(k,n) = Bm[n ldb + k]
// (true: a Linear weight [N][K]) or Bm[k ldb + n].  K % 16 == 0, M % 4 == 0, N % 4 == 0, 16-byte aligned rows.
// Workgroup = 4 waves, tile (16 MT) x 64; wave w owns columns [16 w, +16) and MT accumulator tiles.
enum { EPI_BIAS = 0, EPI_BIAS_RELU_DROP, EPI_BIAS_DROP_RES, EPI_ADD_RES, EPI_PLAIN, EPI_RELU_MASK, EPI_ACCUM };

struct GemmEpi {
  const float* bias;     // [N]
  const float* res;      // [M][ldc]: residual / the saved post-ReLU hidden (EPI_RELU_MASK)
  Drop drop;
  int stream;            // 4 layer + site
  uint8_t* mask;         // optional keep-mask export [M][N]
};

template <int MT, bool AK, bool BK, int EPI>
__global__ __launch_bounds__(256) void tf_gemm(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                               float* __restrict__ Cm, int ldc, int M, int N, int K, int kchunk, GemmEpi ep) {
  constexpr int BM = 16 * MT, BN = 64, BKK = 16, SA = BM + 16, SB = BN + 16;
  __shared__ __attribute__((aligned(16))) float As[BKK][SA];
  __shared__ __attribute__((aligned(16))) float Bs[BKK][SB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  // blockIdx.z splits the reduction axis into chunks of `kchunk`; slice z of the result goes to Cm + z M ldc (weight gradients)
  const int kbeg = blockIdx.z * kchunk, kend = kbeg + kchunk < K ? kbeg + kchunk : K;
  Cm += (long)blockIdx.z * M * ldc;
  f32x4_v acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = f32x4_v{0.f, 0.f, 0.f, 0.f};

  for (int k0 = kbeg; k0 < kend; k0 += BKK) {
    __syncthreads();
    // A tile
    if (AK) {
#pragma unroll
      for (int it = 0; it < (BM * 4 + 255) / 256; ++it) {
        const int idx = tid + it * 256;
        if (idx < BM * 4) {
          const int m = idx >> 2, kq = idx & 3;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (m0 + m < M) v = *(const float4*)(A + (long)(m0 + m) * lda + k0 + kq * 4);
          As[kq * 4 + 0][m] = v.x; As[kq * 4 + 1][m] = v.y; As[kq * 4 + 2][m] = v.z; As[kq * 4 + 3][m] = v.w;
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < (BM * 4 + 255) / 256; ++it) {
        const int idx = tid + it * 256;
        if (idx < BM * 4) {
          const int kk = idx / (BM / 4), mq = idx % (BM / 4);
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (m0 + mq * 4 < M) v = *(const float4*)(A + (long)(k0 + kk) * lda + m0 + mq * 4);
          *(float4*)&As[kk][mq * 4] = v;
        }
      }
    }
    // B tile (64 x 16 = 256 float4: one per lane)
    if (BK) {
      const int n = tid >> 2, kq = tid & 3;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 + n < N) v = *(const float4*)(Bm + (long)(n0 + n) * ldb + k0 + kq * 4);
      Bs[kq * 4 + 0][n] = v.x; Bs[kq * 4 + 1][n] = v.y; Bs[kq * 4 + 2][n] = v.z; Bs[kq * 4 + 3][n] = v.w;
    } else {
      const int kk = tid >> 4, nq = tid & 15;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 + nq * 4 < N) v = *(const float4*)(Bm + (long)(k0 + kk) * ldb + n0 + nq * 4);
      *(float4*)&Bs[kk][nq * 4] = v;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kr = ks * 4 + (lane >> 4);
      const float bf = Bs[kr][wv * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[kr][i * 16 + (lane & 15)], bf, acc[i], 0, 0, 0);
    }
  }

  const int n = n0 + wv * 16 + (lane & 15);
  if (n >= N) return;
  DropKey dk;
  if (EPI == EPI_BIAS_RELU_DROP || EPI == EPI_BIAS_DROP_RES) dk = drop_key(ep.drop, ep.stream);
  const float bias = (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU_DROP || EPI == EPI_BIAS_DROP_RES) ? ep.bias[n] : 0.f;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + i * 16 + 4 * (lane >> 4) + r;
      if (m >= M) continue;
      const long o = (long)m * ldc + n;
      float v = acc[i][r] + bias;
      if (EPI == EPI_BIAS_RELU_DROP) v = fmaxf(v, 0.f);
      if (EPI == EPI_BIAS_RELU_DROP || EPI == EPI_BIAS_DROP_RES) {
        if (dk.thr) {
          const bool kp = drop_keep(dk, (uint32_t)((long)m * N + n));
          v = kp ? v * dk.scale : 0.f;
          if (ep.mask) ep.mask[(long)m * N + n] = kp ? 1 : 0;
        }
      }
      if (EPI == EPI_BIAS_DROP_RES || EPI == EPI_ADD_RES) v += ep.res[o];
      // (the saved hidden is post-ReLU and post-dropout: it is positive exactly where the unit was active AND kept)
      if (EPI == EPI_RELU_MASK) v = ep.res[o] > 0.f ? v * ep.drop.scale : 0.f;
      if (EPI == EPI_ACCUM) v += Cm[o];
      Cm[o] = v;
    }
  }
}

// ---- LayerNorm over E, one wave per token row ---------------------------------------------------------------------------------
template <int NJ>   // 64 NJ >= E: a row lives in NJ registers per lane
__global__ __launch_bounds__(256) void tf_ln_fwd(const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 int M, int E, float eps, float* __restrict__ y, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float x[NJ], s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    x[j] = c < E ? z[(long)row * E + c] : 0.f;
    s += x[j];
  }
  const float mean = wave_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float d = (lane + 64 * j) < E ? x[j] - mean : 0.f;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)E + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < E) y[(long)row * E + c] = (x[j] - mean) * rstd * gamma[c] + beta[c];
  }
  if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// One workgroup per group of 4 RPW rows (RPW per wave).  dz = LayerNorm backward of dy; dzm = dz under the keep mask of the dropout in
// front of the residual add (the gradient of the linear behind it); part[b] receives the clip's column sums
// [bias of that linear: sum dzm | gamma: sum dy xhat | beta: sum dy] at the three given offsets.
template <int NJ, int RPW>
__global__ __launch_bounds__(256) void tf_ln_bwd(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ stats,
                                                 const float* __restrict__ gamma, int E, float* dz, float* dzm,
                                                 float* __restrict__ part, int pstride, int off_bias, int off_gamma, int off_beta,
                                                 Drop drop, int stream) {
  __shared__ float red[4][3][64 * NJ];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x;
  const DropKey dk = drop_key(drop, stream);
  float sb[NJ], sg[NJ], st[NJ], gm[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    sb[j] = sg[j] = st[j] = 0.f;
    gm[j] = (lane + 64 * j) < E ? gamma[lane + 64 * j] : 0.f;
  }
  for (int r = 0; r < RPW; ++r) {
    const long row = (long)b * (4 * RPW) + wv * RPW + r;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float g[NJ], xh[NJ], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      const bool ok = c < E;
      const float d = ok ? dy[row * E + c] : 0.f;
      xh[j] = ok ? (z[row * E + c] - mean) * rstd : 0.f;
      g[j] = d * gm[j];
      s1 += g[j];
      s2 = fmaf(g[j], xh[j], s2);
      sg[j] = fmaf(d, xh[j], sg[j]);
      st[j] += d;
    }
    s1 = wave_sum(s1) / (float)E;
    s2 = wave_sum(s2) / (float)E;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (c < E) {
        const float v = rstd * (g[j] - s1 - xh[j] * s2);
        dz[row * E + c] = v;
        float vm = v;
        if (dk.thr) vm = drop_keep(dk, (uint32_t)(row * E + c)) ? v * dk.scale : 0.f;
        if (dzm != dz) dzm[row * E + c] = vm;
        sb[j] += vm;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < E) { red[wv][0][c] = sb[j]; red[wv][1][c] = sg[j]; red[wv][2][c] = st[j]; }
  }
  __syncthreads();
  float* p = part + (long)b * pstride;
  for (int idx = threadIdx.x; idx < 3 * E; idx += 256) {
    const int w = idx / E, c = idx % E;
    const float s = ((red[0][w][c] + red[1][w][c]) + red[2][w][c]) + red[3][w][c];
    p[(w == 0 ? off_bias : (w == 1 ? off_gamma : off_beta)) + c] = s;
  }
}

// part[b][off + n] = sum over group b's ROWS rows of g[m][n]
template <int ROWS>
__global__ __launch_bounds__(256) void tf_colsum_clip(const float* __restrict__ g, int N, float* __restrict__ part, int pstride, int off) {
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= N) return;
  float s = 0.f;
#pragma unroll 8
  for (int r = 0; r < ROWS; ++r) s += g[((long)b * ROWS + r) * N + n];
  part[(long)b * pstride + off + n] = s;
}

// dst[i] += sum_z part[z n + i], slices in index order
__global__ __launch_bounds__(256) void tf_reduce_split(const float* __restrict__ part, int nsplit, long n, float* __restrict__ dst) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int z = 0; z < nsplit; ++z) s += part[(long)z * n + i];
  dst[i] += s;
}

struct SmallGrads { float* dst[8]; int off[9]; };
// dst[seg][j] += sum_b part[b][off[seg] + j], clips in index order
__global__ __launch_bounds__(256) void tf_reduce_clips(const float* __restrict__ part, int B, int pstride, SmallGrads sg) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= pstride) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += part[(long)b * pstride + j];
#pragma unroll
  for (int seg = 0; seg < 8; ++seg)
    if (j >= sg.off[seg] && j < sg.off[seg + 1] && sg.dst[seg]) sg.dst[seg][j - sg.off[seg]] += s;
}

template <bool AK, bool BK, int EPI>
static void tf_gemm_launch(hipStream_t s, const float* A, int lda, const float* Bm, int ldb, float* Cm, int ldc, int M, int N, int K, const GemmEpi& ep) {
  // taller tiles reuse a weight fragment for more MFMAs but leave fewer workgroups: 32 rows until the grid fills the 256 CUs
  // several times over, then 64, then 128
  if (M >= 8192 && M % 128 == 0) {
    hipLaunchKernelGGL((tf_gemm<8, AK, BK, EPI>), dim3(vn_div_up(N, 64), M / 128), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, ep);
  } else if (M >= 4096 && M % 64 == 0) {
    hipLaunchKernelGGL((tf_gemm<4, AK, BK, EPI>), dim3(vn_div_up(N, 64), M / 64), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, ep);
  } else {
    hipLaunchKernelGGL((tf_gemm<2, AK, BK, EPI>), dim3(vn_div_up(N, 64), vn_div_up(M, 32)), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, ep);
  }
}

// dW[rows][cols] += dY^T X over all M tokens.  One slice: one launch, every workgroup sums all tokens in order.  Several: slices
// of TF_WGRAD_CHUNK tokens into partial matrices at `part`, then one pass adds them in slice order -- fixed for a given batch either way.
static void tf_wgrad_launch(hipStream_t s, int nsplit, float* part, const float* dY, int ldy, const float* X, int ldx, float* dW, int rows, int cols, int M) {
  GemmEpi ep;
  memset(&ep, 0, sizeof(ep));
  if (nsplit <= 1) {
    tf_gemm_launch<false, false, EPI_ACCUM>(s, dY, ldy, X, ldx, dW, cols, rows, cols, M, ep);
    return;
  }
  hipLaunchKernelGGL((tf_gemm<2, false, false, EPI_PLAIN>), dim3(vn_div_up(cols, 64), vn_div_up(rows, 32), nsplit), dim3(256), 0, s, dY, ldy, X, ldx,
                     part, cols, rows, cols, M, TF_WGRAD_CHUNK, ep);
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(tf_reduce_split, dim3(vn_div_up(n, 256)), dim3(256), 0, s, part, nsplit, n, dW);
}

enum { P_INW = 0, P_INB, P_OUTW, P_OUTB, P_L1W, P_L1B, P_L2W, P_L2B, P_N1W, P_N1B, P_N2W, P_N2B, P_COUNT };

}  // namespace
