// Token-wise audio-visual fusion (model.py:116-189): nn.TransformerEncoder over S tokens (the 336 positions of y0 plus the 3 SoundNet
// time steps) of E <= 512 features (the channels), post-norm, ReLU, H heads up to 128 wide, forward and backward.
//
// The tokens are the ROWS of the channels-last activation, so nothing is transposed at the boundary: the first kernel copies the
// view's rows (+ pe) into the fp32 token matrix, the last one copies them out.  In the workspace every clip owns Sp = S rounded up
// to 16 rows, so the token matrices [M = B Sp][.] meet the token GEMM's contract (M % 4 == 0, a weight gradient's reduction axis
// a multiple of 16) whatever S and B are, and the stages between attention are the ones of transformer.hip (tf_common.h).
// The linear products (the six linears of a layer, their data and weight gradients) run in the arithmetic the caller names
// (VINET_TK_MMA_*): tf_gemm on the fp32 MFMA, or tk_gemm_bf16.h on the bf16 MFMA over the same fp32 matrices.  Attention takes a
// mode of its own from the same values: the kernels below, or tk_attn_bf16.h over the same workspace.
// Padding rows: ZERO in the encoder's input and in every gradient matrix, finite (a bias, a LayerNorm of it) in every saved
// activation, so they add exactly 0 to each weight and bias gradient; attention never reads them as keys and writes zeros for them.
//
// Attention for general S: one workgroup per (clip, head, 64 queries), 16 queries per wave, keys / values streamed through LDS
// in tiles, both products on v_mfma_f32_16x16x4_f32.  Forward makes two passes over the keys: scores (written raw into the
// softmax buffer) with the running row maximum and sum, then normalise + dropout + P V.  The softmax rows P [B][H][S][S] are
// SAVED (4 H S^2 bytes per clip and layer); backward reads them in a query-major kernel (dQ) and a key-major kernel (dK, dV),
// each output row summed by one wave in tile order: no atomics.  rowsum(dP P) is taken as rowsum(dAO AO).
// Dropout: the keep masks of tf_common.h; sites 1..3 are indexed by the PADDED row (forward and backward agree, the export kernel
// maps them to [B S][.]), site 0 by the unpadded [B][H][S][S] index.
#include "tf_common.h"
#include "tk_gemm_bf16.h"
#include "tk_attn_bf16.h"

namespace {

constexpr int TK_MAX_S = 1024;
constexpr int TK_MAX_E = 512;     // LayerNorm rows live in 8 registers per lane
constexpr int TK_MAX_D = 128;     // head width
constexpr int TK_BQ = 64;         // queries per workgroup, forward and dQ (keys per workgroup in the dK / dV kernel): 16 per wave
constexpr int TK_BK = 64;         // keys per LDS tile, forward
constexpr int TK_BB = 32;         // keys (dQ kernel) / queries (dK / dV kernel) per LDS tile, backward
constexpr int TK_GROUP = 16;      // rows per partial-sum group of the small gradients (Sp is a multiple of it)
constexpr int TK_LD = TK_MAX_D + 16;

static inline int tk_sp(int S) { return (S + 15) & ~15; }

// ---- boundary: rows of a channels-last view <-> token matrix [B Sp][E] fp32 ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void tk_load_tokens(const T* __restrict__ x, long sB, int ld, const float* __restrict__ pe, int S, int Sp,
                                                      int E, float* __restrict__ X) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= Sp * E) return;
  const int s = idx / E, c = idx - s * E;
  float v = 0.f;
  if (s < S) v = load1<T>(x + (long)b * sB + (long)s * ld + c) + (pe ? pe[idx] : 0.f);
  X[(long)b * Sp * E + idx] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void tk_store_tokens(const float* __restrict__ X, int S, int Sp, int E, T* __restrict__ y, long sB, int ld) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= S * E) return;
  const int s = idx / E, c = idx - s * E;
  store1<T>(y + (long)b * sB + (long)s * ld + c, X[(long)b * Sp * E + idx]);
}

// keep masks of sites 1..3 as bytes [B S][N] (the kernels index them by the padded row)
__global__ __launch_bounds__(256) void tk_export_mask(Drop drop, int stream, int S, int Sp, int N, uint8_t* __restrict__ mask) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= S * N) return;
  const DropKey dk = drop_key(drop, stream);
  mask[(long)b * S * N + idx] = drop_keep(dk, (uint32_t)((long)b * Sp * N + idx)) ? 1 : 0;
}

// ---- attention ----------------------------------------------------------------------------------------------------------------
// MFMA 16x16x4 operand layout (lane = 16 g + n): A[row n][k g], B[k g][col n], result rows 4 g + r (r = 0..3), column n.
// qkv [M][3E] (q | k | v, head h at columns h D); DT = 16-column tiles of the head width (D <= 16 DT, D % 4 == 0).
VN_DEV void tk_load_rows(float* __restrict__ dst, int ldd, const float* __restrict__ src, long lds, int row0, int rows, int S, int nks) {
  // `rows` rows of D = 4 nks floats from src + row lds; rows past the clip's last token repeat it (finite, masked by the caller)
  for (int idx = threadIdx.x; idx < rows * nks; idx += 256) {
    const int r = idx / nks, c4 = idx - r * nks;
    const int row = row0 + r < S ? row0 + r : S - 1;
    *(float4*)(dst + r * ldd + c4 * 4) = *(const float4*)(src + (long)row * lds + c4 * 4);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void tk_attn_fwd(const float* __restrict__ qkv, int S, int Sp, int E, int H, int D, float qscale,
                                                   float* P, float* __restrict__ ao, Drop drop, int stream, uint8_t* __restrict__ mask) {
  __shared__ __attribute__((aligned(16))) float kv[TK_BK * TK_LD];
  __shared__ float ps[4][16][TK_BK + 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, nks = D >> 2;
  const float* base = qkv + (long)b * Sp * 3 * E + h * D;
  const int q0 = blockIdx.x * TK_BQ + wv * 16;
  const long prow0 = ((long)b * H + h) * S;
  const int qrow = q0 + n < S ? q0 + n : S - 1;
  float qf[4 * DT];
#pragma unroll
  for (int ks = 0; ks < 4 * DT; ++ks) qf[ks] = ks < nks ? base[(long)qrow * 3 * E + ks * 4 + g] * qscale : 0.f;

  // pass 1: raw scores into P, running maximum and sum of each row over this lane's columns
  float mx[4], sm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mx[r] = -INFINITY; sm[r] = 0.f; }
  const int ldk = D + 4;
  for (int k0 = 0; k0 < S; k0 += TK_BK) {
    __syncthreads();
    tk_load_rows(kv, ldk, base + E, 3 * E, k0, TK_BK, S, nks);
    __syncthreads();
#pragma unroll 1
    for (int nt = 0; nt < TK_BK / 16; ++nt) {
      f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4 * DT; ++ks)
        if (ks < nks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[ks], kv[(nt * 16 + n) * ldk + ks * 4 + g], acc, 0, 0, 0);
      const int j = k0 + nt * 16 + n;
      if (j < S) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = q0 + 4 * g + r;
          const float s = acc[r];
          if (i < S) P[(prow0 + i) * S + j] = s;
          const float mn = fmaxf(mx[r], s);
          sm[r] = sm[r] * expf(mx[r] - mn) + expf(s - mn);
          mx[r] = mn;
        }
      }
    }
  }
  // the 16 lanes of a row group combine (a lane without a valid column holds (-inf, 0))
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float om = __shfl_xor(mx[r], o, 64), os = __shfl_xor(sm[r], o, 64);
      const float mn = fmaxf(mx[r], om);
      const float a = mx[r] == mn ? 1.f : expf(mx[r] - mn), c = om == mn ? 1.f : expf(om - mn);
      sm[r] = sm[r] * a + os * c;
      mx[r] = mn;
    }
    sm[r] = 1.f / sm[r];
  }

  // pass 2: normalise (P keeps the softmax rows), dropout, O = P V
  const DropKey dk = drop_key(drop, stream);
  const int ldv = D + 16;
  f32x4_v o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += TK_BK) {
    __syncthreads();
    tk_load_rows(kv, ldv, base + 2 * E, 3 * E, k0, TK_BK, S, nks);
#pragma unroll
    for (int nt = 0; nt < TK_BK / 16; ++nt) {
      const int j = k0 + nt * 16 + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + 4 * g + r;
        float p = 0.f;
        if (i < S && j < S) {
          const long e = (prow0 + i) * S + j;
          p = expf(P[e] - mx[r]) * sm[r];      // (this lane wrote P[e] in pass 1)
          P[e] = p;
          if (dk.thr) {
            const bool kp = drop_keep(dk, (uint32_t)e);
            p = kp ? p * dk.scale : 0.f;
            if (mask) mask[e] = kp ? 1 : 0;
          }
        }
        ps[wv][4 * g + r][nt * 16 + n] = p;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < TK_BK / 4; ++ks) {
      const float a = ps[wv][n][ks * 4 + g];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        if (dt * 16 < D) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, kv[(ks * 4 + g) * ldv + dt * 16 + n], o[dt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + n;
    if (d < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + 4 * g + r;
        if (i < Sp) ao[((long)b * Sp + i) * E + h * D + d] = i < S ? o[dt][r] : 0.f;
      }
    }
  }
}

// dot[m][h] = sum_d dAO[m][h D + d] AO[m][h D + d]  ( = sum_j dP[i][j] P[i][j] of the softmax backward)
__global__ __launch_bounds__(256) void tk_attn_dot(const float* __restrict__ dao, const float* __restrict__ ao, long MH, int E, int H, int D,
                                                   float* __restrict__ dot) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= MH) return;
  const long m = t / H;
  const int h = (int)(t - m * H);
  const float4* a = (const float4*)(dao + m * E + h * D);
  const float4* c = (const float4*)(ao + m * E + h * D);
  float s = 0.f;
  for (int d = 0; d < D / 4; ++d) {
    const float4 u = a[d], v = c[d];
    s = fmaf(u.x, v.x, s); s = fmaf(u.y, v.y, s); s = fmaf(u.z, v.z, s); s = fmaf(u.w, v.w, s);
  }
  dot[t] = s;
}

// dQ: one wave per 16 queries, keys in tiles of TK_BB.  dS = P (dP - dot) qscale with dP = (dAO V^T) under the keep mask.
template <int DT>
__global__ __launch_bounds__(256) void tk_attn_bwd_q(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dao,
                                                     const float* __restrict__ dot, int S, int Sp, int E, int H, int D, float qscale,
                                                     float* __restrict__ dqkv, Drop drop, int stream) {
  __shared__ __attribute__((aligned(16))) float kt[TK_BB * TK_LD], vt[TK_BB * TK_LD];
  __shared__ float ps[4][16][TK_BB + 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, nks = D >> 2, ldt = D + 8;
  const float* base = qkv + (long)b * Sp * 3 * E + h * D;
  const int q0 = blockIdx.x * TK_BQ + wv * 16;
  const long prow0 = ((long)b * H + h) * S;
  const int qrow = q0 + n < S ? q0 + n : S - 1;
  float gf[4 * DT], dotr[4];
#pragma unroll
  for (int ks = 0; ks < 4 * DT; ++ks) gf[ks] = ks < nks ? dao[((long)b * Sp + qrow) * E + h * D + ks * 4 + g] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 4 * g + r;
    dotr[r] = dot[((long)b * Sp + (i < S ? i : S - 1)) * H + h];
  }
  const DropKey dk = drop_key(drop, stream);
  f32x4_v dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += TK_BB) {
    __syncthreads();
    tk_load_rows(kt, ldt, base + E, 3 * E, k0, TK_BB, S, nks);
    tk_load_rows(vt, ldt, base + 2 * E, 3 * E, k0, TK_BB, S, nks);
    __syncthreads();
#pragma unroll 1
    for (int nt = 0; nt < TK_BB / 16; ++nt) {
      f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4 * DT; ++ks)
        if (ks < nks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[ks], vt[(nt * 16 + n) * ldt + ks * 4 + g], acc, 0, 0, 0);
      const int j = k0 + nt * 16 + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + 4 * g + r;
        float ds = 0.f;
        if (i < S && j < S) {
          const long e = (prow0 + i) * S + j;
          float m = 1.f;
          if (dk.thr) m = drop_keep(dk, (uint32_t)e) ? dk.scale : 0.f;
          ds = P[e] * (acc[r] * m - dotr[r]) * qscale;
        }
        ps[wv][4 * g + r][nt * 16 + n] = ds;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < TK_BB / 4; ++ks) {
      const float a = ps[wv][n][ks * 4 + g];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        if (dt * 16 < D) dq[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, kt[(ks * 4 + g) * ldt + dt * 16 + n], dq[dt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + n;
    if (d < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = q0 + 4 * g + r;
        if (i < Sp) dqkv[((long)b * Sp + i) * 3 * E + h * D + d] = i < S ? dq[dt][r] : 0.f;
      }
    }
  }
}

// dK, dV: one wave per 16 keys, queries in tiles of TK_BB.  The products are taken transposed ([key][query]) so that the wave's
// output rows are its keys: dP^T = V dAO^T, then dV += Pd^T dAO and dK += dS^T Q.
template <int DT>
__global__ __launch_bounds__(256) void tk_attn_bwd_kv(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dao,
                                                      const float* __restrict__ dot, int S, int Sp, int E, int H, int D, float qscale,
                                                      float* __restrict__ dqkv, Drop drop, int stream) {
  __shared__ __attribute__((aligned(16))) float gt[TK_BB * TK_LD], qt[TK_BB * TK_LD];
  __shared__ float pt[4][16][TK_BB + 4], st[4][16][TK_BB + 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, nks = D >> 2, ldt = D + 8;
  const float* base = qkv + (long)b * Sp * 3 * E + h * D;
  const float* gbase = dao + (long)b * Sp * E + h * D;
  const int j0 = blockIdx.x * TK_BQ + wv * 16;
  const long prow0 = ((long)b * H + h) * S;
  const int krow = j0 + n < S ? j0 + n : S - 1;
  float vf[4 * DT];
#pragma unroll
  for (int ks = 0; ks < 4 * DT; ++ks) vf[ks] = ks < nks ? base[(long)krow * 3 * E + 2 * E + ks * 4 + g] : 0.f;
  const DropKey dk = drop_key(drop, stream);
  f32x4_v dv[DT], dkk[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) { dv[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f}; dkk[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f}; }
  for (int i0 = 0; i0 < S; i0 += TK_BB) {
    __syncthreads();
    tk_load_rows(gt, ldt, gbase, E, i0, TK_BB, S, nks);
    tk_load_rows(qt, ldt, base, 3 * E, i0, TK_BB, S, nks);
    __syncthreads();
#pragma unroll 1
    for (int nt = 0; nt < TK_BB / 16; ++nt) {
      f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4 * DT; ++ks)
        if (ks < nks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[ks], gt[(nt * 16 + n) * ldt + ks * 4 + g], acc, 0, 0, 0);
      const int i = i0 + nt * 16 + n;
      const float dt_i = dot[((long)b * Sp + (i < S ? i : S - 1)) * H + h];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 4 * g + r;
        float pd = 0.f, ds = 0.f;
        if (i < S && j < S) {
          const long e = (prow0 + i) * S + j;
          float m = 1.f;
          if (dk.thr) m = drop_keep(dk, (uint32_t)e) ? dk.scale : 0.f;
          const float p = P[e];
          pd = p * m;
          ds = p * (acc[r] * m - dt_i) * qscale;
        }
        pt[wv][4 * g + r][nt * 16 + n] = pd;
        st[wv][4 * g + r][nt * 16 + n] = ds;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < TK_BB / 4; ++ks) {
      const float a1 = pt[wv][n][ks * 4 + g], a2 = st[wv][n][ks * 4 + g];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        if (dt * 16 < D) {
          dv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, gt[(ks * 4 + g) * ldt + dt * 16 + n], dv[dt], 0, 0, 0);
          dkk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, qt[(ks * 4 + g) * ldt + dt * 16 + n], dkk[dt], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + n;
    if (d < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 4 * g + r;
        if (j < Sp) {
          float* out = dqkv + ((long)b * Sp + j) * 3 * E + h * D + d;
          out[E] = j < S ? dkk[dt][r] : 0.f;
          out[2 * E] = j < S ? dv[dt][r] : 0.f;
        }
      }
    }
  }
}

// ---- split / mean / broadcast (model.py:175-185) ------------------------------------------------------------------------------
// x [B][Sv + Sa][E] -> y [B][Sv][2E]: channels [0, E) the video rows, channels [E, 2E) the mean of the Sa audio rows at every position
template <typename T>
__global__ __launch_bounds__(256) void tk_split_fwd(const T* __restrict__ x, long xsB, int xld, int Sv, int Sa, int E, T* __restrict__ y, long ysB, int yld) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
  if (c >= E) return;
  const T* xb = x + (long)b * xsB;
  float s = 0.f;
  for (int j = 0; j < Sa; ++j) s += load1<T>(xb + (long)(Sv + j) * xld + c);
  s /= (float)Sa;
  for (int pos = blockIdx.y; pos < Sv; pos += gridDim.y) {
    T* yr = y + (long)b * ysB + (long)pos * yld;
    store1<T>(yr + c, load1<T>(xb + (long)pos * xld + c));
    store1<T>(yr + E + c, s);
  }
}

// dx rows [0, Sv) = dy channels [0, E); every audio row = (1 / Sa) * sum over positions (in index order) of dy channels [E, 2E)
template <typename T>
__global__ __launch_bounds__(256) void tk_split_bwd(const T* __restrict__ dy, long ysB, int yld, int Sv, int Sa, int E, T* __restrict__ dx, long xsB, int xld) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
  if (c >= E) return;
  const T* yb = dy + (long)b * ysB;
  T* xb = dx + (long)b * xsB;
  if (blockIdx.y == 0) {
    // (sums of 16 positions, then the sum of those: a fixed order with a shorter rounding chain than one run over all positions)
    float s = 0.f;
    for (int p0 = 0; p0 < Sv; p0 += 16) {
      float part = 0.f;
      for (int pos = p0; pos < Sv && pos < p0 + 16; ++pos) part += load1<T>(yb + (long)pos * yld + E + c);
      s += part;
    }
    s /= (float)Sa;
    for (int j = 0; j < Sa; ++j) store1<T>(xb + (long)(Sv + j) * xld + c, s);
  }
  for (int pos = blockIdx.y; pos < Sv; pos += gridDim.y) store1<T>(xb + (long)pos * xld + c, load1<T>(yb + (long)pos * yld + c));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct Layout {
  long S, Sp, M, E, F, groups;
  // saved per layer (floats)
  long xin, qkv, P, ao, z1, st1, x1, hd, z2, st2, per_layer;
  // scratch (floats)
  long step, dA, dB, dC, dH, dqkv, dot, part, pstride, out, wsplit, nsplit, total;
};
static inline long al4(long n) { return (n + 3) & ~3L; }
static Layout make_layout(const VinetTokenEncoderDesc* d) {
  Layout L;
  L.S = d->S; L.Sp = tk_sp(d->S); L.M = (long)d->B * L.Sp; L.E = d->E; L.F = d->F; L.groups = L.M / TK_GROUP;
  long o = 0;
  L.xin = o; o += L.M * L.E;
  L.qkv = o; o += L.M * 3 * L.E;
  L.P = o; o += al4((long)d->B * d->H * d->S * d->S);
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
  L.nsplit = 1; L.wsplit = 0; L.pstride = 9 * L.E + L.F;
  L.dA = L.dB = L.dC = L.dH = L.dqkv = L.dot = L.part = 0;
  if (d->train) {
    L.dA = o; o += L.M * L.E;
    L.dB = o; o += L.M * L.E;
    L.dC = o; o += L.M * L.E;
    L.dH = o; o += L.M * (L.F > L.E ? L.F : L.E);
    L.dqkv = o; o += L.M * 3 * L.E;
    L.dot = o; o += al4(L.M * d->H);
    L.part = o; o += L.groups * L.pstride;
    L.nsplit = L.M > TF_WGRAD_CHUNK ? (L.M + TF_WGRAD_CHUNK - 1) / TF_WGRAD_CHUNK : 1;
    L.wsplit = o;
    if (L.nsplit > 1) o += L.nsplit * 3 * L.E * (L.F > L.E ? L.F : L.E);
  }
  L.total = o;
  return L;
}

static int check_desc(const VinetTokenEncoderDesc* d, const char* who) {
  VN_CHECK_ARG(d, "%s: null descriptor", who);
  VN_CHECK_ARG(d->dtype == VINET_F32 || d->dtype == VINET_BF16 || d->dtype == VINET_F32S, "%s: bad dtype %d", who, d->dtype);
  VN_CHECK_ARG(d->B > 0 && d->L > 0 && d->H > 0, "%s: B, L, H must be positive", who);
  VN_CHECK_ARG(d->S >= 1 && d->S <= TK_MAX_S, "%s: S = %d tokens per clip must be in [1, %d]", who, d->S, TK_MAX_S);
  VN_CHECK_ARG(d->E > 0 && d->E % 16 == 0 && d->E <= TK_MAX_E, "%s: E = %d must be a multiple of 16 and <= %d", who, d->E, TK_MAX_E);
  VN_CHECK_ARG(d->F > 0 && d->F % 16 == 0, "%s: F = %d must be a multiple of 16", who, d->F);
  VN_CHECK_ARG(d->E % d->H == 0 && d->E / d->H <= TK_MAX_D && (d->E / d->H) % 4 == 0,
               "%s: head width E / H = %d / %d must be an integer multiple of 4 and <= %d", who, d->E, d->H, TK_MAX_D);
  VN_CHECK_ARG(d->p >= 0.f && d->p < 1.f, "%s: dropout p = %f", who, (double)d->p);
  // (the widest token matrix is [B Sp][max(3E, F)]: its elements are also the counter of the keep masks of sites 1..3)
  VN_CHECK_ARG((long)d->B * tk_sp(d->S) * (3 * d->E > d->F ? 3 * d->E : d->F) < (1L << 31) && (long)d->B * d->H * d->S * d->S < (1L << 32),
               "%s: B = %d clips of %d tokens exceed the kernels' 32-bit row and mask indices", who, d->B, d->S);
  return 0;
}

static bool tensor_ok(const VinetTensor* t, const VinetTokenEncoderDesc* d) {
  return t && t->ptr && t->B == d->B && (long)t->T * t->H * t->W == d->S && t->C == d->E && t->ld >= t->C;
}

static int check_mma(int32_t mma, const char* who) {
  VN_CHECK_ARG(mma == VINET_TK_MMA_F32 || mma == VINET_TK_MMA_BF16X3 || mma == VINET_TK_MMA_BF16,
               "%s: mma = %d is not VINET_TK_MMA_F32 (0), _BF16X3 (1) or _BF16 (2)", who, mma);
  return 0;
}

static int check_attn(int32_t attn, const char* who) {
  VN_CHECK_ARG(attn == VINET_TK_MMA_F32 || attn == VINET_TK_MMA_BF16X3 || attn == VINET_TK_MMA_BF16,
               "%s: attn = %d is not VINET_TK_MMA_F32 (0), _BF16X3 (1) or _BF16 (2)", who, attn);
  return 0;
}

#define TK_BY_WIDTH(D, CALL)                 \
  do {                                       \
    if ((D) <= 16) { CALL(1); }              \
    else if ((D) <= 32) { CALL(2); }         \
    else if ((D) <= 64) { CALL(4); }         \
    else { CALL(8); }                        \
  } while (0)

}  // namespace

// (the bf16 GEMMs read and write the fp32 matrices of the fp32 ones: one layout, one size, whatever the mode)
extern "C" int64_t vinet_token_encoder_workspace_attn(const VinetTokenEncoderDesc* d, int32_t mma, int32_t attn) {
  if (check_desc(d, "token_encoder_workspace") || check_mma(mma, "token_encoder_workspace") || check_attn(attn, "token_encoder_workspace")) return -1;
  return make_layout(d).total * (int64_t)sizeof(float);
}
extern "C" int64_t vinet_token_encoder_workspace_mma(const VinetTokenEncoderDesc* d, int32_t mma) {
  return vinet_token_encoder_workspace_attn(d, mma, VINET_TK_MMA_F32);
}
extern "C" int64_t vinet_token_encoder_workspace(const VinetTokenEncoderDesc* d) { return vinet_token_encoder_workspace_mma(d, VINET_TK_MMA_F32); }

// mask export layout (bytes): per layer [site 0: B H S S | site 1: B S E | site 2: B S F | site 3: B S E]
static inline long tk_mask_layer_bytes(const VinetTokenEncoderDesc* d) {
  const long MS = (long)d->B * d->S;
  return (long)d->B * d->H * d->S * d->S + 2 * MS * d->E + MS * d->F;
}

extern "C" int vinet_token_encoder_fwd_attn(const VinetTokenEncoderDesc* d, int32_t mma, int32_t attn, const VinetTensor* x, const VinetTensor* y,
                                            void* stream) {
  if (check_desc(d, "token_encoder_fwd") || check_mma(mma, "token_encoder_fwd") || check_attn(attn, "token_encoder_fwd")) return -1;
  VN_CHECK_ARG(tensor_ok(x, d) && tensor_ok(y, d), "token_encoder_fwd: x / y must be [B][T H W = S][C = E] channels-last with ld >= C");
  VN_CHECK_ARG(d->params && d->pe && d->ws && (((uintptr_t)d->ws) & 15) == 0, "token_encoder_fwd: params, pe and a 16-byte aligned workspace are required");
  const Layout L = make_layout(d);
  VN_CHECK_ARG(d->ws_bytes >= L.total * (int64_t)sizeof(float), "token_encoder_fwd: workspace too small");
  const bool dropping = d->p > 0.f;
  VN_CHECK_ARG(!dropping || d->step, "token_encoder_fwd: dropout needs the device step counter");
  for (int i = 0; i < d->L * P_COUNT; ++i) VN_CHECK_ARG(d->params[i], "token_encoder_fwd: parameter %d of layer %d is null", i % P_COUNT, i / P_COUNT);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)d->ws;
  const int M = (int)L.M, E = d->E, F = d->F, H = d->H, D = E / H, B = d->B, S = d->S, Sp = (int)L.Sp;
  const Drop drop = tf_make_drop(d->p, d->seed, (const int64_t*)(ws + L.step));
  if (dropping) hipLaunchKernelGGL(tf_step_kernel, dim3(1), dim3(64), 0, s, d->step, (int64_t*)(ws + L.step));
  const float qscale = 1.f / sqrtf((float)D);
  float* cur = ws + L.xin;      // layer 0's input slot
  const dim3 lgrid(vn_div_up((long)Sp * E, 256), B), sgrid(vn_div_up((long)S * E, 256), B);
  if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tk_load_tokens<bf16_t>, lgrid, dim3(256), 0, s, (const bf16_t*)x->ptr, (long)x->sB, x->ld, d->pe, S, Sp, E, cur);
  else hipLaunchKernelGGL(tk_load_tokens<float>, lgrid, dim3(256), 0, s, (const float*)x->ptr, (long)x->sB, x->ld, d->pe, S, Sp, E, cur);
  const dim3 agrid(vn_div_up(S, TK_BQ), H, B);
  for (int l = 0; l < d->L; ++l) {
    const float* const* P = (const float* const*)d->params + (long)l * P_COUNT;
    float* sv = ws + (d->train ? l : 0) * L.per_layer;
    uint8_t* mk = (d->masks && dropping) ? d->masks + (long)l * tk_mask_layer_bytes(d) : nullptr;
    GemmEpi ep;
    ep.drop = drop; ep.mask = nullptr;
    // (eval mode has ONE slot; the layer's input is then `out`, which this layer's last LayerNorm overwrites after its readers)
    const float* xin = cur;
    ep.bias = P[P_INB]; ep.res = nullptr; ep.stream = 0;
    tk_gemm_launch<true, true, EPI_BIAS>(mma, s, xin, E, P[P_INW], E, sv + L.qkv, 3 * E, M, 3 * E, E, ep);
#define TK_FWD(DT) hipLaunchKernelGGL(tk_attn_fwd<DT>, agrid, dim3(256), 0, s, sv + L.qkv, S, Sp, E, H, D, qscale, sv + L.P, sv + L.ao, drop, 4 * l + 0, mk)
    if (attn == VINET_TK_MMA_F32) TK_BY_WIDTH(D, TK_FWD);
    else tk_attn_fwd_bf16_launch(attn, s, sv + L.qkv, B, S, Sp, E, H, qscale, sv + L.P, sv + L.ao, drop, 4 * l + 0, mk);
#undef TK_FWD
    ep.bias = P[P_OUTB]; ep.res = xin; ep.stream = 4 * l + 1;
    tk_gemm_launch<true, true, EPI_BIAS_DROP_RES>(mma, s, sv + L.ao, E, P[P_OUTW], E, sv + L.z1, E, M, E, E, ep);
    hipLaunchKernelGGL(tf_ln_fwd<8>, dim3(vn_div_up(M, 4)), dim3(256), 0, s, sv + L.z1, P[P_N1W], P[P_N1B], M, E, d->eps, sv + L.x1, sv + L.st1);
    ep.bias = P[P_L1B]; ep.res = nullptr; ep.stream = 4 * l + 2;
    tk_gemm_launch<true, true, EPI_BIAS_RELU_DROP>(mma, s, sv + L.x1, E, P[P_L1W], E, sv + L.hd, F, M, F, E, ep);
    ep.bias = P[P_L2B]; ep.res = sv + L.x1; ep.stream = 4 * l + 3;
    tk_gemm_launch<true, true, EPI_BIAS_DROP_RES>(mma, s, sv + L.hd, F, P[P_L2W], F, sv + L.z2, E, M, E, F, ep);
    float* nxt = (d->train && l + 1 < d->L) ? ws + (l + 1) * L.per_layer + L.xin : ws + L.out;
    hipLaunchKernelGGL(tf_ln_fwd<8>, dim3(vn_div_up(M, 4)), dim3(256), 0, s, sv + L.z2, P[P_N2W], P[P_N2B], M, E, d->eps, nxt, sv + L.st2);
    cur = nxt;
    if (mk) {
      uint8_t* m1 = mk + (long)B * H * S * S;
      uint8_t* m2 = m1 + (long)B * S * E;
      uint8_t* m3 = m2 + (long)B * S * F;
      hipLaunchKernelGGL(tk_export_mask, sgrid, dim3(256), 0, s, drop, 4 * l + 1, S, Sp, E, m1);
      hipLaunchKernelGGL(tk_export_mask, dim3(vn_div_up((long)S * F, 256), B), dim3(256), 0, s, drop, 4 * l + 2, S, Sp, F, m2);
      hipLaunchKernelGGL(tk_export_mask, sgrid, dim3(256), 0, s, drop, 4 * l + 3, S, Sp, E, m3);
    }
  }
  if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tk_store_tokens<bf16_t>, sgrid, dim3(256), 0, s, cur, S, Sp, E, (bf16_t*)y->ptr, (long)y->sB, y->ld);
  else hipLaunchKernelGGL(tk_store_tokens<float>, sgrid, dim3(256), 0, s, cur, S, Sp, E, (float*)y->ptr, (long)y->sB, y->ld);
  return vn_launch_status("token_encoder_fwd");
}

extern "C" int vinet_token_encoder_bwd_attn(const VinetTokenEncoderDesc* d, int32_t mma, int32_t attn, const VinetTensor* dy, const VinetTensor* dx,
                                            void* stream) {
  if (check_desc(d, "token_encoder_bwd") || check_mma(mma, "token_encoder_bwd") || check_attn(attn, "token_encoder_bwd")) return -1;
  VN_CHECK_ARG(d->train, "token_encoder_bwd: the forward pass must have run with train = 1 (it saves the layers' state)");
  VN_CHECK_ARG(tensor_ok(dy, d) && (!dx || tensor_ok(dx, d)), "token_encoder_bwd: dy / dx must be [B][T H W = S][C = E] channels-last with ld >= C");
  VN_CHECK_ARG(d->params && d->grads && d->ws && (((uintptr_t)d->ws) & 15) == 0, "token_encoder_bwd: params, grads and the forward's workspace are required");
  const Layout L = make_layout(d);
  VN_CHECK_ARG(d->ws_bytes >= L.total * (int64_t)sizeof(float), "token_encoder_bwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)d->ws;
  const int M = (int)L.M, E = d->E, F = d->F, H = d->H, D = E / H, B = d->B, S = d->S, Sp = (int)L.Sp, NG = (int)L.groups;
  const Drop drop = tf_make_drop(d->p, d->seed, (const int64_t*)(ws + L.step));
  const bool dropping = drop.thr != 0;
  const float qscale = 1.f / sqrtf((float)D);
  float *dOut = ws + L.dA, *dZ = ws + L.dB, *dZm = dropping ? ws + L.dC : ws + L.dB;
  float *dH = ws + L.dH, *dQKV = ws + L.dqkv, *part = ws + L.part, *dot = ws + L.dot, *wpart = ws + L.wsplit;
  // dX1 (the gradient entering the first LayerNorm) takes the head of dQKV's buffer: dQKV is written by the attention backward,
  // after that LayerNorm's backward has consumed dX1
  float* dX1 = dQKV;
  const int ps = (int)L.pstride, ns = (int)L.nsplit;
  // partial-sum columns: in_proj_bias | out_proj.bias | linear1.bias | linear2.bias | norm1.w | norm1.b | norm2.w | norm2.b
  const int oINB = 0, oOUTB = 3 * E, oL1B = 4 * E, oL2B = 4 * E + F, oN1W = 5 * E + F, oN1B = 6 * E + F, oN2W = 7 * E + F, oN2B = 8 * E + F;
  const dim3 lgrid(vn_div_up((long)Sp * E, 256), B), sgrid(vn_div_up((long)S * E, 256), B), agrid(vn_div_up(S, TK_BQ), H, B);
  if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tk_load_tokens<bf16_t>, lgrid, dim3(256), 0, s, (const bf16_t*)dy->ptr, (long)dy->sB, dy->ld, (const float*)nullptr, S, Sp, E, dOut);
  else hipLaunchKernelGGL(tk_load_tokens<float>, lgrid, dim3(256), 0, s, (const float*)dy->ptr, (long)dy->sB, dy->ld, (const float*)nullptr, S, Sp, E, dOut);
  for (int l = d->L - 1; l >= 0; --l) {
    const float* const* P = (const float* const*)d->params + (long)l * P_COUNT;
    float* const* G = (float* const*)d->grads + (long)l * P_COUNT;
    float* sv = ws + l * L.per_layer;
    GemmEpi ep;
    ep.drop = drop; ep.bias = nullptr; ep.res = nullptr; ep.stream = 0; ep.mask = nullptr;
    // LayerNorm 2: dOut -> dZ (residual path) and dZm (linear2's output gradient)
    hipLaunchKernelGGL((tf_ln_bwd<8, TK_GROUP / 4>), dim3(NG), dim3(256), 0, s, dOut, sv + L.z2, sv + L.st2, P[P_N2W], E, dZ, dZm, part, ps, oL2B, oN2W, oN2B, drop, 4 * l + 3);
    // linear2: dH = (dZm W2) under the ReLU / dropout of the hidden;  dW2 += dZm^T hidden
    ep.res = sv + L.hd;
    tk_gemm_launch<true, false, EPI_RELU_MASK>(mma, s, dZm, E, P[P_L2W], F, dH, F, M, F, E, ep);
    if (G[P_L2W]) tk_wgrad_launch(mma, s, ns, wpart, dZm, E, sv + L.hd, F, G[P_L2W], E, F, M);
    hipLaunchKernelGGL(tf_colsum_clip<TK_GROUP>, dim3(vn_div_up(F, 256), NG), dim3(256), 0, s, dH, F, part, ps, oL1B);
    // linear1: dX1 = dH W1 + dZ;  dW1 += dH^T x1
    ep.res = dZ;
    tk_gemm_launch<true, false, EPI_ADD_RES>(mma, s, dH, F, P[P_L1W], E, dX1, E, M, E, F, ep);
    if (G[P_L1W]) tk_wgrad_launch(mma, s, ns, wpart, dH, F, sv + L.x1, E, G[P_L1W], F, E, M);
    // LayerNorm 1
    hipLaunchKernelGGL((tf_ln_bwd<8, TK_GROUP / 4>), dim3(NG), dim3(256), 0, s, dX1, sv + L.z1, sv + L.st1, P[P_N1W], E, dZ, dZm, part, ps, oOUTB, oN1W, oN1B, drop, 4 * l + 1);
    // attention projection: dAO = dZm Wo (into dH's buffer);  dWo += dZm^T ao
    float* dAO = dH;
    tk_gemm_launch<true, false, EPI_PLAIN>(mma, s, dZm, E, P[P_OUTW], E, dAO, E, M, E, E, ep);
    if (G[P_OUTW]) tk_wgrad_launch(mma, s, ns, wpart, dZm, E, sv + L.ao, E, G[P_OUTW], E, E, M);
    hipLaunchKernelGGL(tk_attn_dot, dim3(vn_div_up((long)M * H, 256)), dim3(256), 0, s, dAO, sv + L.ao, (long)M * H, E, H, D, dot);
#define TK_BWD(DT)                                                                                                                                    \
  hipLaunchKernelGGL(tk_attn_bwd_q<DT>, agrid, dim3(256), 0, s, sv + L.qkv, sv + L.P, dAO, dot, S, Sp, E, H, D, qscale, dQKV, drop, 4 * l + 0);   \
  hipLaunchKernelGGL(tk_attn_bwd_kv<DT>, agrid, dim3(256), 0, s, sv + L.qkv, sv + L.P, dAO, dot, S, Sp, E, H, D, qscale, dQKV, drop, 4 * l + 0)
    if (attn == VINET_TK_MMA_F32) TK_BY_WIDTH(D, TK_BWD);
    else tk_attn_bwd_bf16_launch(attn, s, sv + L.qkv, sv + L.P, dAO, dot, B, S, Sp, E, H, qscale, dQKV, drop, 4 * l + 0);
#undef TK_BWD
    hipLaunchKernelGGL(tf_colsum_clip<TK_GROUP>, dim3(vn_div_up(3 * E, 256), NG), dim3(256), 0, s, dQKV, 3 * E, part, ps, oINB);
    // QKV projection: dXin = dQKV Win + dZ;  dWin += dQKV^T xin
    ep.res = dZ;
    tk_gemm_launch<true, false, EPI_ADD_RES>(mma, s, dQKV, 3 * E, P[P_INW], E, dOut, E, M, E, 3 * E, ep);
    if (G[P_INW]) tk_wgrad_launch(mma, s, ns, wpart, dQKV, 3 * E, sv + L.xin, E, G[P_INW], 3 * E, E, M);
    SmallGrads sg;
    const int pidx[8] = {P_INB, P_OUTB, P_L1B, P_L2B, P_N1W, P_N1B, P_N2W, P_N2B};
    const int offs[9] = {oINB, oOUTB, oL1B, oL2B, oN1W, oN1B, oN2W, oN2B, ps};
    for (int i = 0; i < 8; ++i) sg.dst[i] = G[pidx[i]];
    for (int i = 0; i < 9; ++i) sg.off[i] = offs[i];
    hipLaunchKernelGGL(tf_reduce_clips, dim3(vn_div_up(ps, 256)), dim3(256), 0, s, part, NG, ps, sg);
  }
  if (dx) {
    if (d->dtype == VINET_BF16) hipLaunchKernelGGL(tk_store_tokens<bf16_t>, sgrid, dim3(256), 0, s, dOut, S, Sp, E, (bf16_t*)dx->ptr, (long)dx->sB, dx->ld);
    else hipLaunchKernelGGL(tk_store_tokens<float>, sgrid, dim3(256), 0, s, dOut, S, Sp, E, (float*)dx->ptr, (long)dx->sB, dx->ld);
  }
  return vn_launch_status("token_encoder_bwd");
}

extern "C" int vinet_token_encoder_fwd_mma(const VinetTokenEncoderDesc* d, int32_t mma, const VinetTensor* x, const VinetTensor* y, void* stream) {
  return vinet_token_encoder_fwd_attn(d, mma, VINET_TK_MMA_F32, x, y, stream);
}
extern "C" int vinet_token_encoder_bwd_mma(const VinetTokenEncoderDesc* d, int32_t mma, const VinetTensor* dy, const VinetTensor* dx, void* stream) {
  return vinet_token_encoder_bwd_attn(d, mma, VINET_TK_MMA_F32, dy, dx, stream);
}
extern "C" int vinet_token_encoder_fwd(const VinetTokenEncoderDesc* d, const VinetTensor* x, const VinetTensor* y, void* stream) {
  return vinet_token_encoder_fwd_mma(d, VINET_TK_MMA_F32, x, y, stream);
}
extern "C" int vinet_token_encoder_bwd(const VinetTokenEncoderDesc* d, const VinetTensor* dy, const VinetTensor* dx, void* stream) {
  return vinet_token_encoder_bwd_mma(d, VINET_TK_MMA_F32, dy, dx, stream);
}

// ---- one product (vinet_token_gemm) -------------------------------------------------------------------------------------------
namespace {
struct TkGemmArgs {
  int mma;
  const float *A, *B;
  float* C;
  int lda, ldb, ldc, M, N, K;
  GemmEpi ep;
};

template <bool AK, bool BK, int EPI>
static int tk_one_product(const TkGemmArgs& g, hipStream_t s) {
  const int nsplit = (!AK && g.K > TF_WGRAD_CHUNK) ? (g.K + TF_WGRAD_CHUNK - 1) / TF_WGRAD_CHUNK : 1;
  if (nsplit <= 1) {
    tk_gemm_launch<AK, BK, EPI>(g.mma, s, g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.M, g.N, g.K, g.ep);
    return vn_launch_status("token_gemm");
  }
  float* part = nullptr;
  const hipError_t e = hipMalloc((void**)&part, (size_t)nsplit * g.M * g.N * sizeof(float));
  VN_CHECK_ARG(e == hipSuccess, "token_gemm: no memory for %d partial matrices of %d x %d: %s", nsplit, g.M, g.N, hipGetErrorString(e));
  tk_wgrad_slices(g.mma, s, nsplit, part, g.A, g.lda, g.B, g.ldb, g.M, g.N, g.K);
  hipLaunchKernelGGL(tk_reduce_epi<EPI>, dim3(vn_div_up((long)g.M * g.N, 256)), dim3(256), 0, s, part, nsplit, g.M, g.N, g.C, g.ldc, g.ep);
  const int rc = vn_launch_status("token_gemm");
  (void)hipStreamSynchronize(s);
  (void)hipFree(part);
  return rc;
}

template <bool AK, bool BK>
static int tk_one_product_epi(int epi, const TkGemmArgs& g, hipStream_t s) {
  switch (epi) {
    case 0: return tk_one_product<AK, BK, EPI_PLAIN>(g, s);
    case 1: return tk_one_product<AK, BK, EPI_BIAS>(g, s);
    case 2: return tk_one_product<AK, BK, EPI_BIAS_RELU_DROP>(g, s);     // (no dropout: ep.drop.thr == 0)
    case 3: return tk_one_product<AK, BK, EPI_ADD_RES>(g, s);
    default: return tk_one_product<AK, BK, EPI_ACCUM>(g, s);
  }
}
}  // namespace

extern "C" int vinet_token_gemm(int32_t mma, int32_t form, int32_t epi, const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc,
                                int32_t M, int32_t N, int32_t K, const float* bias, const float* res, void* stream) {
  if (check_mma(mma, "token_gemm")) return -1;
  VN_CHECK_ARG(form >= 0 && form <= 2, "token_gemm: form = %d is not 0 (A[m][k] B[n][k]), 1 (A[m][k] B[k][n]) or 2 (A[k][m] B[k][n])", form);
  VN_CHECK_ARG(epi >= 0 && epi <= 4, "token_gemm: epi = %d is not 0 (plain), 1 (+ bias), 2 (relu(. + bias)), 3 (+ res) or 4 (C +=)", epi);
  VN_CHECK_ARG(M > 0 && M % 4 == 0, "token_gemm: M = %d must be a positive multiple of 4", M);
  VN_CHECK_ARG(N > 0 && N % 4 == 0, "token_gemm: N = %d must be a positive multiple of 4", N);
  VN_CHECK_ARG(K > 0 && K % 16 == 0, "token_gemm: K = %d must be a positive multiple of 16", K);
  VN_CHECK_ARG(A && B && C, "token_gemm: null matrix");
  const int wa = form == 2 ? M : K, wb = form == 0 ? K : N;
  VN_CHECK_ARG(lda >= wa && ldb >= wb && ldc >= N, "token_gemm: row strides lda = %d, ldb = %d, ldc = %d are below the widths %d, %d, %d", lda, ldb, ldc, wa, wb, N);
  VN_CHECK_ARG(lda % 4 == 0 && ldb % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) & 15) == 0, "token_gemm: rows of A and B must be 16-byte aligned (lda = %d, ldb = %d)", lda, ldb);
  VN_CHECK_ARG((epi != 1 && epi != 2) || bias, "token_gemm: epi = %d needs bias", epi);
  VN_CHECK_ARG(epi != 3 || res, "token_gemm: epi = 3 needs res");
  TkGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.mma = mma; g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  g.ep.bias = bias; g.ep.res = res; g.ep.drop = tf_make_drop(0.f, 0, nullptr);
  hipStream_t s = (hipStream_t)stream;
  if (form == 0) return tk_one_product_epi<true, true>(epi, g, s);
  if (form == 1) return tk_one_product_epi<true, false>(epi, g, s);
  return tk_one_product_epi<false, false>(epi, g, s);
}

// ---- one attention stage (vinet_token_attn_fwd / _bwd): no dropout, caller-owned matrices in the workspace's row layout ------------
static int attn_args_ok(int32_t attn, int32_t B, int32_t S, int32_t E, int32_t H, const char* who) {
  if (check_attn(attn, who)) return -1;
  VN_CHECK_ARG(B > 0 && H > 0, "%s: B = %d and H = %d must be positive", who, B, H);
  VN_CHECK_ARG(S >= 1 && S <= TK_MAX_S, "%s: S = %d tokens per clip must be in [1, %d]", who, S, TK_MAX_S);
  VN_CHECK_ARG(E > 0 && E % 16 == 0 && E <= TK_MAX_E, "%s: E = %d must be a multiple of 16 and <= %d", who, E, TK_MAX_E);
  VN_CHECK_ARG(E % H == 0 && E / H <= TK_MAX_D && (E / H) % 4 == 0, "%s: head width E / H = %d / %d must be an integer multiple of 4 and <= %d", who, E,
               H, TK_MAX_D);
  VN_CHECK_ARG((long)B * tk_sp(S) * 3 * E < (1L << 31) && (long)B * H * S * S < (1L << 32),
               "%s: B = %d clips of %d tokens exceed the kernels' 32-bit row and mask indices", who, B, S);
  return 0;
}
static inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" int vinet_token_attn_fwd(int32_t attn, const float* qkv, int32_t B, int32_t S, int32_t E, int32_t H, float* P, float* ao, void* stream) {
  if (attn_args_ok(attn, B, S, E, H, "token_attn_fwd")) return -1;
  VN_CHECK_ARG(qkv && P && ao, "token_attn_fwd: null matrix");
  VN_CHECK_ARG(al16(qkv) && al16(ao) && (((uintptr_t)P) & 3) == 0, "token_attn_fwd: qkv and ao must be 16-byte aligned, P 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int Sp = tk_sp(S), D = E / H;
  const float qscale = 1.f / sqrtf((float)D);
  const Drop drop = tf_make_drop(0.f, 0, nullptr);
  const dim3 agrid(vn_div_up(S, TK_BQ), H, B);
  uint8_t* mk = nullptr;
#define TK_FWD(DT) hipLaunchKernelGGL(tk_attn_fwd<DT>, agrid, dim3(256), 0, s, qkv, S, Sp, E, H, D, qscale, P, ao, drop, 0, mk)
  if (attn == VINET_TK_MMA_F32) TK_BY_WIDTH(D, TK_FWD);
  else tk_attn_fwd_bf16_launch(attn, s, qkv, B, S, Sp, E, H, qscale, P, ao, drop, 0, mk);
#undef TK_FWD
  return vn_launch_status("token_attn_fwd");
}

extern "C" int vinet_token_attn_bwd(int32_t attn, const float* qkv, const float* P, const float* dao, const float* ao, int32_t B, int32_t S, int32_t E,
                                    int32_t H, float* dot, float* dqkv, void* stream) {
  if (attn_args_ok(attn, B, S, E, H, "token_attn_bwd")) return -1;
  VN_CHECK_ARG(qkv && P && dao && ao && dot && dqkv, "token_attn_bwd: null matrix");
  VN_CHECK_ARG(al16(qkv) && al16(dao) && al16(ao) && al16(dqkv) && ((((uintptr_t)P) | ((uintptr_t)dot)) & 3) == 0,
               "token_attn_bwd: qkv, dao, ao and dqkv must be 16-byte aligned, P and dot 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int Sp = tk_sp(S), D = E / H;
  const long M = (long)B * Sp;
  const float qscale = 1.f / sqrtf((float)D);
  const Drop drop = tf_make_drop(0.f, 0, nullptr);
  const dim3 agrid(vn_div_up(S, TK_BQ), H, B);
  hipLaunchKernelGGL(tk_attn_dot, dim3(vn_div_up(M * H, 256)), dim3(256), 0, s, dao, ao, M * H, E, H, D, dot);
#define TK_BWD(DT)                                                                                                  \
  hipLaunchKernelGGL(tk_attn_bwd_q<DT>, agrid, dim3(256), 0, s, qkv, P, dao, dot, S, Sp, E, H, D, qscale, dqkv, drop, 0);   \
  hipLaunchKernelGGL(tk_attn_bwd_kv<DT>, agrid, dim3(256), 0, s, qkv, P, dao, dot, S, Sp, E, H, D, qscale, dqkv, drop, 0)
  if (attn == VINET_TK_MMA_F32) TK_BY_WIDTH(D, TK_BWD);
  else tk_attn_bwd_bf16_launch(attn, s, qkv, P, dao, dot, B, S, Sp, E, H, qscale, dqkv, drop, 0);
#undef TK_BWD
  return vn_launch_status("token_attn_bwd");
}

static int split_args_ok(const VinetTensor* x, const VinetTensor* y, int32_t n_audio, const char* who) {
  VN_CHECK_ARG(x && y && x->ptr && y->ptr, "%s: null tensor", who);
  const long Sx = (long)x->T * x->H * x->W, Sy = (long)y->T * y->H * y->W;
  VN_CHECK_ARG(n_audio >= 1 && Sx == Sy + n_audio && Sy >= 1, "%s: %ld token rows must be %ld positions + %d audio rows", who, Sx, Sy, n_audio);
  VN_CHECK_ARG(x->B == y->B && x->B > 0 && x->C > 0 && y->C == 2 * x->C && x->ld >= x->C && y->ld >= y->C,
               "%s: tokens [B][Sv + Sa][E] and the fused tensor [B][Sv][2E] do not fit (C = %d / %d)", who, x->C, y->C);
  return 0;
}

extern "C" int vinet_token_split_fwd(const VinetTensor* x, int32_t dtype, int32_t n_audio, const VinetTensor* y, void* stream) {
  VN_CHECK_ARG(dtype == VINET_F32 || dtype == VINET_BF16 || dtype == VINET_F32S, "token_split_fwd: bad dtype %d", dtype);
  if (split_args_ok(x, y, n_audio, "token_split_fwd")) return -1;
  const int Sv = y->T * y->H * y->W, E = x->C;
  const dim3 grid(vn_div_up(E, 256), Sv < 64 ? Sv : 64, x->B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == VINET_BF16) hipLaunchKernelGGL(tk_split_fwd<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x->ptr, (long)x->sB, x->ld, Sv, n_audio, E, (bf16_t*)y->ptr, (long)y->sB, y->ld);
  else hipLaunchKernelGGL(tk_split_fwd<float>, grid, dim3(256), 0, s, (const float*)x->ptr, (long)x->sB, x->ld, Sv, n_audio, E, (float*)y->ptr, (long)y->sB, y->ld);
  return vn_launch_status("token_split_fwd");
}

extern "C" int vinet_token_split_bwd(const VinetTensor* dy, int32_t dtype, int32_t n_audio, const VinetTensor* dx, void* stream) {
  VN_CHECK_ARG(dtype == VINET_F32 || dtype == VINET_BF16 || dtype == VINET_F32S, "token_split_bwd: bad dtype %d", dtype);
  if (split_args_ok(dx, dy, n_audio, "token_split_bwd")) return -1;
  const int Sv = dy->T * dy->H * dy->W, E = dx->C;
  const dim3 grid(vn_div_up(E, 256), Sv < 64 ? Sv : 64, dx->B);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == VINET_BF16) hipLaunchKernelGGL(tk_split_bwd<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)dy->ptr, (long)dy->sB, dy->ld, Sv, n_audio, E, (bf16_t*)dx->ptr, (long)dx->sB, dx->ld);
  else hipLaunchKernelGGL(tk_split_bwd<float>, grid, dim3(256), 0, s, (const float*)dy->ptr, (long)dy->sB, dy->ld, Sv, n_audio, E, (float*)dx->ptr, (long)dx->sB, dx->ld);
  return vn_launch_status("token_split_bwd");
}
