// AViNet transformer fusion (model.py:8-69, 211-221, 239-247): nn.TransformerEncoder over S = 32 tokens (the channels of
// conv_in_1x1) x E = 336 features (the 4 x 7 x 12 positions), post-norm, ReLU, nhead heads, forward and backward.
//
// The stack is latency-bound (45 MFLOP per clip and layer), so each layer is a short chain of fused stages on fp32 token
// matrices [M = 32 B][E] that live in the caller's workspace:
//   forward   QKV GEMM+bias | attention per (clip, head) | out-proj GEMM+bias+dropout+residual | LayerNorm |
//             linear1 GEMM+bias+ReLU+dropout | linear2 GEMM+bias+dropout+residual | LayerNorm                       7 launches
//   backward  LayerNorm bwd (+ per-clip partial sums of gamma / beta / the bias behind it) | data GEMMs with the ReLU / residual
//             epilogues | weight GEMMs that ADD into the gradient buffers | attention bwd | one reduce of the per-clip partials  14 launches
// The channels-last activation [B][E][S] (fp32 or bf16) is transposed by the first and the last kernel's loads and stores.
// All GEMMs run on v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation, in every context (a bf16 context differs in
// the two boundary kernels only).  Softmax rows and LayerNorm statistics are fp32 and SAVED by forward (16 KB + 512 B per clip
// and layer); dropout keep masks are RECOMPUTED by backward from (seed, step, layer, site, element).
// Determinism: a weight gradient is one workgroup's sequential sum over all tokens (above 512 tokens: over 512-token slices,
// whose partial matrices are added in slice order); the small gradients are per-clip partial sums reduced over clips in index
// order.  No atomics anywhere.
#include "common.h"

namespace {

constexpr int TF_S = 32;         // tokens per clip (conv_out_1x1 fixes 32 channels, model.py:213)
constexpr int TF_MAX_E = 384;    // LayerNorm rows live in 6 registers per lane
constexpr int TF_MAX_D = 96;     // head width (LDS tiles of the attention kernels)
constexpr int TF_DP = TF_MAX_D + 1;
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

// ---- boundary kernels: channels-last [B][E positions][S channels] (T) <-> token matrix [B*S][E] fp32 ---------------------------
template <typename T>
__global__ __launch_bounds__(256) void tf_load_tokens(const T* __restrict__ x, long sB, int ld, const float* __restrict__ pe, int E,
                                                      float* __restrict__ X) {
  __shared__ float tile[32][33];
  const int b = blockIdx.y, f0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int f = f0 + ty * 4 + r;
    tile[ty * 4 + r][tx] = f < E ? load1<T>(x + (long)b * sB + (long)f * ld + tx) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = ty * 4 + r, f = f0 + tx;
    if (f < E) X[((long)b * TF_S + c) * E + f] = tile[tx][c] + (pe ? pe[c * E + f] : 0.f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void tf_store_tokens(const float* __restrict__ X, int E, T* __restrict__ y, long sB, int ld) {
  __shared__ float tile[32][33];
  const int b = blockIdx.y, f0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = ty * 4 + r, f = f0 + tx;
    tile[c][tx] = f < E ? X[((long)b * TF_S + c) * E + f] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int f = f0 + ty * 4 + r;
    if (f < E) store1<T>(y + (long)b * sB + (long)f * ld + tx, tile[tx][ty * 4 + r]);
  }
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

// ---- attention, one workgroup per (clip, head) ------------------------------------------------------------------------------
// qkv [M][3E] (q | k | v, head h at columns h D), P [B][H][S][S] = softmax rows (saved, before dropout), ao [M][E].
__global__ __launch_bounds__(256) void tf_attn_fwd(const float* __restrict__ qkv, int E, int H, int D, float qscale, float* __restrict__ P,
                                                   float* __restrict__ ao, Drop drop, int stream, uint8_t* __restrict__ mask) {
  __shared__ float q[TF_S][TF_DP], k[TF_S][TF_DP], v[TF_S][TF_DP], pd[TF_S][TF_S + 1];
  const int b = blockIdx.x / H, h = blockIdx.x % H, tid = threadIdx.x;
  const float* base = qkv + (long)b * TF_S * 3 * E + h * D;
  for (int idx = tid; idx < TF_S * D; idx += 256) {
    const int s = idx / D, d = idx % D;
    const float* p = base + (long)s * 3 * E + d;
    q[s][d] = p[0] * qscale; k[s][d] = p[E]; v[s][d] = p[2 * E];
  }
  __syncthreads();
  const int i = tid >> 3, j0 = tid & 7;
  float sc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) sc[r] = 0.f;
  for (int d = 0; d < D; ++d) {
    const float qv = q[i][d];
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = fmaf(qv, k[j0 + 8 * r][d], sc[r]);
  }
  float mx = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) { sc[r] = expf(sc[r] - mx); sum += sc[r]; }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) sum += __shfl_xor(sum, o, 64);
  const float inv = 1.f / sum;
  const DropKey dk = drop_key(drop, stream);
  const long prow = ((long)blockIdx.x * TF_S + i) * TF_S;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + 8 * r;
    float p = sc[r] * inv;
    P[prow + j] = p;
    if (dk.thr) {
      const bool kp = drop_keep(dk, (uint32_t)(prow + j));
      p = kp ? p * dk.scale : 0.f;
      if (mask) mask[prow + j] = kp ? 1 : 0;
    }
    pd[i][j] = p;
  }
  __syncthreads();
  for (int d = j0; d < D; d += 8) {
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < TF_S; ++j) o = fmaf(pd[i][j], v[j][d], o);
    ao[((long)b * TF_S + i) * E + h * D + d] = o;
  }
}

__global__ __launch_bounds__(256) void tf_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dao,
                                                   int E, int H, int D, float qscale, float* __restrict__ dqkv, Drop drop, int stream) {
  __shared__ float q[TF_S][TF_DP], k[TF_S][TF_DP], v[TF_S][TF_DP], go[TF_S][TF_DP], pd[TF_S][TF_S + 1], ds[TF_S][TF_S + 1];
  const int b = blockIdx.x / H, h = blockIdx.x % H, tid = threadIdx.x;
  const float* base = qkv + (long)b * TF_S * 3 * E + h * D;
  for (int idx = tid; idx < TF_S * D; idx += 256) {
    const int s = idx / D, d = idx % D;
    const float* p = base + (long)s * 3 * E + d;
    q[s][d] = p[0]; k[s][d] = p[E]; v[s][d] = p[2 * E];
    go[s][d] = dao[((long)b * TF_S + s) * E + h * D + d];
  }
  __syncthreads();
  const int i = tid >> 3, j0 = tid & 7;
  const DropKey dk = drop_key(drop, stream);
  const long prow = ((long)blockIdx.x * TF_S + i) * TF_S;
  float dp[4], pr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dp[r] = 0.f;
  for (int d = 0; d < D; ++d) {
    const float g = go[i][d];
#pragma unroll
    for (int r = 0; r < 4; ++r) dp[r] = fmaf(g, v[j0 + 8 * r][d], dp[r]);
  }
  float dot = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + 8 * r;
    pr[r] = P[prow + j];
    float m = 1.f;
    if (dk.thr) m = drop_keep(dk, (uint32_t)(prow + j)) ? dk.scale : 0.f;
    pd[i][j] = pr[r] * m;
    dp[r] *= m;
    dot = fmaf(dp[r], pr[r], dot);
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) dot += __shfl_xor(dot, o, 64);
#pragma unroll
  for (int r = 0; r < 4; ++r) ds[i][j0 + 8 * r] = pr[r] * (dp[r] - dot) * qscale;
  __syncthreads();
  // row `i` of dQ, dK, dV (i is a query index for dQ and a key index for dK / dV)
  float* out = dqkv + ((long)b * TF_S + i) * 3 * E + h * D;
  for (int d = j0; d < D; d += 8) {
    float dq = 0.f, dkk = 0.f, dv = 0.f;
#pragma unroll
    for (int j = 0; j < TF_S; ++j) {
      dq = fmaf(ds[i][j], k[j][d], dq);
      dkk = fmaf(ds[j][i], q[j][d], dkk);
      dv = fmaf(pd[j][i], go[j][d], dv);
    }
    out[d] = dq; out[E + d] = dkk; out[2 * E + d] = dv;
  }
}

// ---- LayerNorm over E, one wave per token row ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tf_ln_fwd(const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 int M, int E, float eps, float* __restrict__ y, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float x[6], s = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int c = lane + 64 * j;
    x[j] = c < E ? z[(long)row * E + c] : 0.f;
    s += x[j];
  }
  const float mean = wave_sum(s) / (float)E;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const float d = (lane + 64 * j) < E ? x[j] - mean : 0.f;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)E + eps);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int c = lane + 64 * j;
    if (c < E) y[(long)row * E + c] = (x[j] - mean) * rstd * gamma[c] + beta[c];
  }
  if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// One workgroup per clip (32 rows; 8 per wave).  dz = LayerNorm backward of dy; dzm = dz under the keep mask of the dropout in
// front of the residual add (the gradient of the linear behind it); part[b] receives the clip's column sums
// [bias of that linear: sum dzm | gamma: sum dy xhat | beta: sum dy] at the three given offsets.
__global__ __launch_bounds__(256) void tf_ln_bwd(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ stats,
                                                 const float* __restrict__ gamma, int E, float* dz, float* dzm,
                                                 float* __restrict__ part, int pstride, int off_bias, int off_gamma, int off_beta,
                                                 Drop drop, int stream) {
  __shared__ float red[4][3][TF_MAX_E];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x;
  const DropKey dk = drop_key(drop, stream);
  float sb[6], sg[6], st[6], gm[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    sb[j] = sg[j] = st[j] = 0.f;
    gm[j] = (lane + 64 * j) < E ? gamma[lane + 64 * j] : 0.f;
  }
  for (int r = 0; r < 8; ++r) {
    const long row = (long)b * TF_S + wv * 8 + r;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float g[6], xh[6], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
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
    for (int j = 0; j < 6; ++j) {
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
  for (int j = 0; j < 6; ++j) {
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

// part[b][off + n] = sum over the clip's 32 rows of g[m][n]
__global__ __launch_bounds__(256) void tf_colsum_clip(const float* __restrict__ g, int N, float* __restrict__ part, int pstride, int off) {
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= N) return;
  float s = 0.f;
#pragma unroll 8
  for (int r = 0; r < TF_S; ++r) s += g[((long)b * TF_S + r) * N + n];
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

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct Layout {
  long M, E, F;
  // saved per layer (floats)
  long xin, qkv, P, ao, z1, st1, x1, hd, z2, st2, per_layer;
  // scratch (floats)
  long step, dA, dB, dC, dH, dqkv, part, pstride, scratch, out, wsplit, nsplit, total;
};
static inline long al4(long n) { return (n + 3) & ~3L; }
static Layout make_layout(const VinetTransformerDesc* d) {
  Layout L;
  L.M = (long)d->B * d->S; L.E = d->E; L.F = d->F;
  long o = 0;
  L.xin = o; o += L.M * L.E;
  L.qkv = o; o += L.M * 3 * L.E;
  L.P = o; o += (long)d->B * d->H * d->S * d->S;
  L.ao = o; o += L.M * L.E;
  L.z1 = o; o += L.M * L.E;
  L.st1 = o; o += al4(2 * L.M);
  L.x1 = o; o += L.M * L.E;
  L.hd = o; o += L.M * L.F;
  L.z2 = o; o += L.M * L.E;
  L.st2 = o; o += al4(2 * L.M);
  L.per_layer = o;
  const long slots = d->train ? d->L : 1;
  o = slots * L.per_layer;
  L.step = o; o += 4;
  L.out = o; o += L.M * L.E;                       // the layer output (next layer's xin in eval mode / the stack's result)
  L.scratch = o;
  L.nsplit = 1; L.wsplit = 0;
  if (d->train) {
    L.dA = o; o += L.M * L.E;
    L.dB = o; o += L.M * L.E;
    L.dC = o; o += L.M * L.E;
    L.dH = o; o += L.M * (L.F > L.E ? L.F : L.E);
    L.dqkv = o; o += L.M * 3 * L.E;
    L.pstride = 9 * L.E + L.F;
    L.part = o; o += (long)d->B * L.pstride;
    // weight gradients of many clips: the token axis is cut into TF_WGRAD_CHUNK-token slices, one partial matrix each
    // (no sequential sum runs over more than one slice: at 992 tokens in one launch linear1's weight gradient was 4.07 x the torch
    //  model's own fp32 error from the fp64 result, tests/test_gpu_transformer_shapes.py)
    L.nsplit = L.M > TF_WGRAD_CHUNK ? (L.M + TF_WGRAD_CHUNK - 1) / TF_WGRAD_CHUNK : 1;
    L.wsplit = o;
    if (L.nsplit > 1) o += L.nsplit * 3 * L.E * (L.F > L.E ? L.F : L.E);
  }
  L.total = o;
  return L;
}

static int check_desc(const VinetTransformerDesc* d, const char* who) {
  VN_CHECK_ARG(d, "%s: null descriptor", who);
  VN_CHECK_ARG(d->dtype == VINET_F32 || d->dtype == VINET_BF16 || d->dtype == VINET_F32S, "%s: bad dtype %d", who, d->dtype);
  VN_CHECK_ARG(d->B > 0 && d->L > 0 && d->H > 0, "%s: B, L, H must be positive", who);
  VN_CHECK_ARG(d->S == TF_S, "%s: %d tokens per clip (the kernels are built for %d)", who, d->S, TF_S);
  VN_CHECK_ARG(d->E > 0 && d->E % 16 == 0 && d->E <= TF_MAX_E, "%s: E = %d must be a multiple of 16 and <= %d", who, d->E, TF_MAX_E);
  VN_CHECK_ARG(d->F > 0 && d->F % 16 == 0, "%s: F = %d must be a multiple of 16", who, d->F);
  VN_CHECK_ARG(d->E % d->H == 0 && d->E / d->H <= TF_MAX_D, "%s: head width E / H = %d / %d must be an integer <= %d", who, d->E, d->H, TF_MAX_D);
  VN_CHECK_ARG(d->p >= 0.f && d->p < 1.f, "%s: dropout p = %f", who, (double)d->p);
  return 0;
}

static Drop make_drop(const VinetTransformerDesc* d, const float* ws, const Layout& L) {
  Drop r;
  const bool on = d->p > 0.f;
  r.step = (const int64_t*)(ws + L.step);
  r.seed_lo = (uint32_t)d->seed; r.seed_hi = (uint32_t)(d->seed >> 32);
  double t = (double)d->p * 4294967296.0;
  r.thr = on ? (uint32_t)(t < 1.0 ? 1.0 : (t > 4294967295.0 ? 4294967295.0 : t)) : 0u;
  r.scale = on ? 1.f / (1.f - d->p) : 1.f;
  return r;
}

template <bool AK, bool BK, int EPI>
static void gemm(hipStream_t s, const float* A, int lda, const float* Bm, int ldb, float* Cm, int ldc, int M, int N, int K, const GemmEpi& ep) {
  // taller tiles reuse a weight fragment for more MFMAs but leave fewer workgroups: 32 rows until the grid fills the 256 CUs
  // several times over (N = 336 is 6 column tiles), then 64, then 128
  if (M >= 8192 && M % 128 == 0) {
    hipLaunchKernelGGL((tf_gemm<8, AK, BK, EPI>), dim3(vn_div_up(N, 64), M / 128), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, ep);
  } else if (M >= 4096 && M % 64 == 0) {
    hipLaunchKernelGGL((tf_gemm<4, AK, BK, EPI>), dim3(vn_div_up(N, 64), M / 64), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, ep);
  } else {
    hipLaunchKernelGGL((tf_gemm<2, AK, BK, EPI>), dim3(vn_div_up(N, 64), vn_div_up(M, 32)), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, ep);
  }
}

// dW[rows][cols] += dY^T X over all M tokens.  Up to 16 clips: one launch, every workgroup sums all tokens in order.  Many clips: slices
// of TF_WGRAD_CHUNK tokens into partial matrices, then one pass adds them in slice order -- fixed for a given batch either way.
static void wgrad(hipStream_t s, const Layout& L, float* ws, const float* dY, int ldy, const float* X, int ldx, float* dW, int rows, int cols, int M) {
  GemmEpi ep;
  memset(&ep, 0, sizeof(ep));
  if (L.nsplit <= 1) {
    gemm<false, false, EPI_ACCUM>(s, dY, ldy, X, ldx, dW, cols, rows, cols, M, ep);
    return;
  }
  float* part = ws + L.wsplit;
  hipLaunchKernelGGL((tf_gemm<2, false, false, EPI_PLAIN>), dim3(vn_div_up(cols, 64), vn_div_up(rows, 32), (int)L.nsplit), dim3(256), 0, s, dY, ldy, X, ldx,
                     part, cols, rows, cols, M, TF_WGRAD_CHUNK, ep);
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(tf_reduce_split, dim3(vn_div_up(n, 256)), dim3(256), 0, s, part, (int)L.nsplit, n, dW);
}

enum { P_INW = 0, P_INB, P_OUTW, P_OUTB, P_L1W, P_L1B, P_L2W, P_L2B, P_N1W, P_N1B, P_N2W, P_N2B, P_COUNT };

static bool tensor_ok(const VinetTensor* t, const VinetTransformerDesc* d) {
  return t && t->ptr && t->B == d->B && (long)t->T * t->H * t->W == d->E && t->C == d->S && t->ld >= t->C;
}

}  // namespace

extern "C" int64_t vinet_transformer_workspace(const VinetTransformerDesc* d) {
  if (check_desc(d, "transformer_workspace")) return -1;
  return make_layout(d).total * (int64_t)sizeof(float);
}

// mask export layout (bytes): per layer [site 0: B H S S | site 1: M E | site 2: M F | site 3: M E]
static inline long mask_layer_bytes(const VinetTransformerDesc* d) {
  const long M = (long)d->B * d->S;
  return (long)d->B * d->H * d->S * d->S + 2 * M * d->E + M * d->F;
}

extern "C" int vinet_transformer_fwd(const VinetTransformerDesc* d, const VinetTensor* x, const VinetTensor* y, void* stream) {
  if (check_desc(d, "transformer_fwd")) return -1;
  VN_CHECK_ARG(tensor_ok(x, d) && tensor_ok(y, d), "transformer_fwd: x / y must be [B][T H W = E][C = S] channels-last");
  VN_CHECK_ARG(d->params && d->pe && d->ws && (((uintptr_t)d->ws) & 15) == 0, "transformer_fwd: params, pe and a 16-byte aligned workspace are required");
  const Layout L = make_layout(d);
  VN_CHECK_ARG(d->ws_bytes >= L.total * (int64_t)sizeof(float), "transformer_fwd: workspace too small");
  const bool dropping = d->p > 0.f;
  VN_CHECK_ARG(!dropping || d->step, "transformer_fwd: dropout needs the device step counter");
  for (int i = 0; i < d->L * P_COUNT; ++i) VN_CHECK_ARG(d->params[i], "transformer_fwd: parameter %d of layer %d is null", i % P_COUNT, i / P_COUNT);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)d->ws;
  const int M = (int)L.M, E = d->E, F = d->F, H = d->H, D = E / H, B = d->B;
  const Drop drop = make_drop(d, ws, L);
  if (dropping) hipLaunchKernelGGL(tf_step_kernel, dim3(1), dim3(64), 0, s, d->step, (int64_t*)(ws + L.step));
  const float qscale = 1.f / sqrtf((float)D);
  const dim3 tgrid(vn_div_up(E, 32), B);
  float* cur = ws + L.xin;      // layer 0's input slot
  if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tf_load_tokens<bf16_t>, tgrid, dim3(256), 0, s, (const bf16_t*)x->ptr, (long)x->sB, x->ld, d->pe, E, cur);
  else hipLaunchKernelGGL(tf_load_tokens<float>, tgrid, dim3(256), 0, s, (const float*)x->ptr, (long)x->sB, x->ld, d->pe, E, cur);
  for (int l = 0; l < d->L; ++l) {
    const float* const* P = (const float* const*)d->params + (long)l * P_COUNT;
    float* sv = ws + (d->train ? l : 0) * L.per_layer;
    uint8_t* mk = (d->masks && dropping) ? d->masks + (long)l * mask_layer_bytes(d) : nullptr;
    uint8_t* mk1 = mk ? mk + (long)B * H * TF_S * TF_S : nullptr;
    uint8_t* mk2 = mk ? mk1 + (long)M * E : nullptr;
    uint8_t* mk3 = mk ? mk2 + (long)M * F : nullptr;
    GemmEpi ep;
    ep.drop = drop;
    // (eval mode has ONE slot; the layer's input is then `out`, which this layer's last LayerNorm overwrites after its readers)
    const float* xin = cur;
    ep.bias = P[P_INB]; ep.res = nullptr; ep.stream = 0; ep.mask = nullptr;
    gemm<true, true, EPI_BIAS>(s, xin, E, P[P_INW], E, sv + L.qkv, 3 * E, M, 3 * E, E, ep);
    hipLaunchKernelGGL(tf_attn_fwd, dim3(B * H), dim3(256), 0, s, sv + L.qkv, E, H, D, qscale, sv + L.P, sv + L.ao, drop, 4 * l + 0, mk);
    ep.bias = P[P_OUTB]; ep.res = xin; ep.stream = 4 * l + 1; ep.mask = mk1;
    gemm<true, true, EPI_BIAS_DROP_RES>(s, sv + L.ao, E, P[P_OUTW], E, sv + L.z1, E, M, E, E, ep);
    hipLaunchKernelGGL(tf_ln_fwd, dim3(vn_div_up(M, 4)), dim3(256), 0, s, sv + L.z1, P[P_N1W], P[P_N1B], M, E, d->eps, sv + L.x1, sv + L.st1);
    ep.bias = P[P_L1B]; ep.res = nullptr; ep.stream = 4 * l + 2; ep.mask = mk2;
    gemm<true, true, EPI_BIAS_RELU_DROP>(s, sv + L.x1, E, P[P_L1W], E, sv + L.hd, F, M, F, E, ep);
    ep.bias = P[P_L2B]; ep.res = sv + L.x1; ep.stream = 4 * l + 3; ep.mask = mk3;
    gemm<true, true, EPI_BIAS_DROP_RES>(s, sv + L.hd, F, P[P_L2W], F, sv + L.z2, E, M, E, F, ep);
    float* nxt = (d->train && l + 1 < d->L) ? ws + (l + 1) * L.per_layer + L.xin : ws + L.out;
    hipLaunchKernelGGL(tf_ln_fwd, dim3(vn_div_up(M, 4)), dim3(256), 0, s, sv + L.z2, P[P_N2W], P[P_N2B], M, E, d->eps, nxt, sv + L.st2);
    cur = nxt;
  }
  if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tf_store_tokens<bf16_t>, tgrid, dim3(256), 0, s, cur, E, (bf16_t*)y->ptr, (long)y->sB, y->ld);
  else hipLaunchKernelGGL(tf_store_tokens<float>, tgrid, dim3(256), 0, s, cur, E, (float*)y->ptr, (long)y->sB, y->ld);
  return vn_launch_status("transformer_fwd");
}

extern "C" int vinet_transformer_bwd(const VinetTransformerDesc* d, const VinetTensor* dy, const VinetTensor* dx, void* stream) {
  if (check_desc(d, "transformer_bwd")) return -1;
  VN_CHECK_ARG(d->train, "transformer_bwd: the forward pass must have run with train = 1 (it saves the layers' state)");
  VN_CHECK_ARG(tensor_ok(dy, d) && (!dx || tensor_ok(dx, d)), "transformer_bwd: dy / dx must be [B][T H W = E][C = S] channels-last");
  VN_CHECK_ARG(d->params && d->grads && d->ws && (((uintptr_t)d->ws) & 15) == 0, "transformer_bwd: params, grads and the forward's workspace are required");
  const Layout L = make_layout(d);
  VN_CHECK_ARG(d->ws_bytes >= L.total * (int64_t)sizeof(float), "transformer_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)d->ws;
  const int M = (int)L.M, E = d->E, F = d->F, H = d->H, D = E / H, B = d->B;
  const Drop drop = make_drop(d, ws, L);
  const bool dropping = drop.thr != 0;
  const float qscale = 1.f / sqrtf((float)D);
  const dim3 tgrid(vn_div_up(E, 32), B);
  float *dOut = ws + L.dA, *dZ = ws + L.dB, *dZm = dropping ? ws + L.dC : ws + L.dB;
  float *dH = ws + L.dH, *dQKV = ws + L.dqkv, *part = ws + L.part;
  // dX1 (the gradient entering the first LayerNorm) takes the head of dQKV's buffer: dQKV is written by the attention backward,
  // after that LayerNorm's backward has consumed dX1
  float* dX1 = dQKV;
  const int ps = (int)L.pstride;
  // partial-sum columns: in_proj_bias | out_proj.bias | linear1.bias | linear2.bias | norm1.w | norm1.b | norm2.w | norm2.b
  const int oINB = 0, oOUTB = 3 * E, oL1B = 4 * E, oL2B = 4 * E + F, oN1W = 5 * E + F, oN1B = 6 * E + F, oN2W = 7 * E + F, oN2B = 8 * E + F;
  if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tf_load_tokens<bf16_t>, tgrid, dim3(256), 0, s, (const bf16_t*)dy->ptr, (long)dy->sB, dy->ld, (const float*)nullptr, E, dOut);
  else hipLaunchKernelGGL(tf_load_tokens<float>, tgrid, dim3(256), 0, s, (const float*)dy->ptr, (long)dy->sB, dy->ld, (const float*)nullptr, E, dOut);
  for (int l = d->L - 1; l >= 0; --l) {
    const float* const* P = (const float* const*)d->params + (long)l * P_COUNT;
    float* const* G = (float* const*)d->grads + (long)l * P_COUNT;
    float* sv = ws + l * L.per_layer;
    GemmEpi ep;
    ep.drop = drop; ep.bias = nullptr; ep.res = nullptr; ep.stream = 0; ep.mask = nullptr;
    // LayerNorm 2: dOut -> dZ (residual path) and dZm (linear2's output gradient)
    hipLaunchKernelGGL(tf_ln_bwd, dim3(B), dim3(256), 0, s, dOut, sv + L.z2, sv + L.st2, P[P_N2W], E, dZ, dZm, part, ps, oL2B, oN2W, oN2B, drop, 4 * l + 3);
    // linear2: dH = (dZm W2) under the ReLU / dropout of the hidden;  dW2 += dZm^T hidden
    ep.res = sv + L.hd;
    gemm<true, false, EPI_RELU_MASK>(s, dZm, E, P[P_L2W], F, dH, F, M, F, E, ep);
    if (G[P_L2W]) wgrad(s, L, ws, dZm, E, sv + L.hd, F, G[P_L2W], E, F, M);
    hipLaunchKernelGGL(tf_colsum_clip, dim3(vn_div_up(F, 256), B), dim3(256), 0, s, dH, F, part, ps, oL1B);
    // linear1: dX1 = dH W1 + dZ;  dW1 += dH^T x1
    ep.res = dZ;
    gemm<true, false, EPI_ADD_RES>(s, dH, F, P[P_L1W], E, dX1, E, M, E, F, ep);
    if (G[P_L1W]) wgrad(s, L, ws, dH, F, sv + L.x1, E, G[P_L1W], F, E, M);
    // LayerNorm 1
    hipLaunchKernelGGL(tf_ln_bwd, dim3(B), dim3(256), 0, s, dX1, sv + L.z1, sv + L.st1, P[P_N1W], E, dZ, dZm, part, ps, oOUTB, oN1W, oN1B, drop, 4 * l + 1);
    // attention projection: dAO = dZm Wo (into dH's buffer);  dWo += dZm^T ao
    float* dAO = dH;
    gemm<true, false, EPI_PLAIN>(s, dZm, E, P[P_OUTW], E, dAO, E, M, E, E, ep);
    if (G[P_OUTW]) wgrad(s, L, ws, dZm, E, sv + L.ao, E, G[P_OUTW], E, E, M);
    hipLaunchKernelGGL(tf_attn_bwd, dim3(B * H), dim3(256), 0, s, sv + L.qkv, sv + L.P, dAO, E, H, D, qscale, dQKV, drop, 4 * l + 0);
    hipLaunchKernelGGL(tf_colsum_clip, dim3(vn_div_up(3 * E, 256), B), dim3(256), 0, s, dQKV, 3 * E, part, ps, oINB);
    // QKV projection: dXin = dQKV Win + dZ;  dWin += dQKV^T xin
    ep.res = dZ;
    gemm<true, false, EPI_ADD_RES>(s, dQKV, 3 * E, P[P_INW], E, dOut, E, M, E, 3 * E, ep);
    if (G[P_INW]) wgrad(s, L, ws, dQKV, 3 * E, sv + L.xin, E, G[P_INW], 3 * E, E, M);
    SmallGrads sg;
    const int pidx[8] = {P_INB, P_OUTB, P_L1B, P_L2B, P_N1W, P_N1B, P_N2W, P_N2B};
    const int offs[9] = {oINB, oOUTB, oL1B, oL2B, oN1W, oN1B, oN2W, oN2B, ps};
    for (int i = 0; i < 8; ++i) sg.dst[i] = G[pidx[i]];
    for (int i = 0; i < 9; ++i) sg.off[i] = offs[i];
    hipLaunchKernelGGL(tf_reduce_clips, dim3(vn_div_up(ps, 256)), dim3(256), 0, s, part, B, ps, sg);
  }
  if (dx) {
    if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tf_store_tokens<bf16_t>, tgrid, dim3(256), 0, s, dOut, E, (bf16_t*)dx->ptr, (long)dx->sB, dx->ld);
    else hipLaunchKernelGGL(tf_store_tokens<float>, tgrid, dim3(256), 0, s, dOut, E, (float*)dx->ptr, (long)dx->sB, dx->ld);
  }
  return vn_launch_status("transformer_bwd");
}
