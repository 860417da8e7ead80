// The token encoder's linear products on the bf16 MFMA (v_mfma_f32_16x16x32_bf16): the same fp32 matrices tf_gemm reads, the same
// three operand orientations and the same seven epilogues, with the operands rounded to bf16 WHILE they are staged into LDS.
//
// Arithmetic (template parameter MODE, the values of VINET_TK_MMA_*):
//   TKM_BF16    every operand element a becomes hi(a) = bf16(a), round to nearest even (v_cvt_pk_bf16_f32); product = sum hi hi.
//   TKM_BF16X3  hi(a) as above and lo(a) = bf16(a - hi(a)) (the subtraction is exact in fp32); product = sum (hi_a hi_b + hi_a lo_b
//               + lo_a hi_b): the two-term split of VINET_F32S (include/vinet_hip.h), three MFMAs per k-step.
// Accumulation is fp32 inside the MFMA; every result element is one sequential sum over k in index order (32 per MFMA), so a
// result depends on the data alone.  Weight gradients keep tf_gemm's scheme: slices of TF_WGRAD_CHUNK rows over blockIdx.z into
// partial matrices, added in slice order by tf_reduce_split.
//
// Workgroup = 4 waves, tile (64 WM) x 64, k-step 32.  Wave w owns rows [16 WM w, +16 WM) of the tile and all 64 columns: WM x 4
// accumulator tiles.  LDS holds both operand tiles as [row][32 k] bf16 with 80-byte rows (a lane's fragment = the 8 consecutive k
// at 8 (lane >> 4) of row lane & 15: one 16-byte read; rows 80 bytes apart put the 16 rows of a lane group on 16 different
// 16-byte bank slots), one plane for hi and one for lo.  Two LDS buffers: the global loads of tile t + 1 are issued before the
// MFMAs of tile t and converted / written behind them, one barrier per k-step.
// An operand whose k axis is strided in memory (B of the data gradient, both operands of the weight gradient) is transposed on
// the way in: a lane loads four columns of two consecutive k rows and writes four (k, k + 1) pairs, 16 lanes on 16 consecutive
// dwords of a row.
//
// The kernels carry VN_NO_PK_F32 (common.h): a - hi(a) on register pairs is where hipcc forms packed fp32 subtractions.
#pragma once
#include "tf_common.h"

namespace {

enum { TKM_F32 = VINET_TK_MMA_F32, TKM_BF16X3 = VINET_TK_MMA_BF16X3, TKM_BF16 = VINET_TK_MMA_BF16 };

constexpr int TKG_BN = 64;     // tile columns
constexpr int TKG_BK = 32;     // k per step = one MFMA
constexpr int TKG_LD = 40;     // bf16 per LDS row: 32 + 8 of padding (80 bytes)
constexpr int TKG_TALL_M = 4096;   // from this many rows on, 128-row tiles (WM = 2)

// ---- epilogue: what tf_gemm does with one accumulator element (same operations in the same order) --------------------------------
template <int EPI>
VN_DEV void tk_epilogue(float acc, int m, int n, int N, float* __restrict__ Cm, int ldc, float bias, const DropKey& dk, const GemmEpi& ep) {
  const long o = (long)m * ldc + n;
  float v = acc + bias;
  if (EPI == EPI_BIAS_RELU_DROP) v = fmaxf(v, 0.f);
  if (EPI == EPI_BIAS_RELU_DROP || EPI == EPI_BIAS_DROP_RES) {
    if (dk.thr) {
      const bool kp = drop_keep(dk, (uint32_t)((long)m * N + n));
      v = kp ? v * dk.scale : 0.f;
      if (ep.mask) ep.mask[(long)m * N + n] = kp ? 1 : 0;
    }
  }
  if (EPI == EPI_BIAS_DROP_RES || EPI == EPI_ADD_RES) v += ep.res[o];
  if (EPI == EPI_RELU_MASK) v = ep.res[o] > 0.f ? v * ep.drop.scale : 0.f;
  if (EPI == EPI_ACCUM) v += Cm[o];
  Cm[o] = v;
}
template <int EPI> VN_DEV bool tk_epi_drops() { return EPI == EPI_BIAS_RELU_DROP || EPI == EPI_BIAS_DROP_RES; }
template <int EPI> VN_DEV bool tk_epi_bias() { return EPI == EPI_BIAS || EPI == EPI_BIAS_RELU_DROP || EPI == EPI_BIAS_DROP_RES; }

// ---- staging ------------------------------------------------------------------------------------------------------------------
// two fp32 -> one dword of hi (element x in the low half) and, for the split, one of lo
template <bool X3>
VN_DEV void tk_split2(float x, float y, uint32_t& h, uint32_t& l) {
  h = pack2bf(x, y);
  if (X3) l = pack2bf(x - __uint_as_float(h << 16), y - __uint_as_float(h & 0xffff0000u));
}

// global -> registers: the tile rows [row0, row0 + ROWS) x k [k0, k0 + 32) of an operand, zero outside [0, nrows) x [., kend).
// KC: k is contiguous in memory (P[row ld + k]); a lane takes 8 k of one row.  Otherwise P[k ld + row]: 4 rows of 2 k.
template <int ROWS, bool KC>
VN_DEV void tk_fetch(float4 (&r)[ROWS / 64][2], const float* __restrict__ P, int ld, int row0, int nrows, int k0, int kend, int tid) {
#pragma unroll
  for (int it = 0; it < ROWS / 64; ++it) {
    const int idx = tid + it * 256;
    r[it][0] = r[it][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KC) {
      const int row = row0 + (idx >> 2), k = k0 + (idx & 3) * 8;
      if (row < nrows && k < kend) {
        const float* p = P + (long)row * ld + k;
        r[it][0] = *(const float4*)p;
        r[it][1] = *(const float4*)(p + 4);
      }
    } else {
      const int k = k0 + (idx & 15) * 2, row = row0 + (idx >> 4) * 4;
      if (row < nrows && k < kend) {
        const float* p = P + (long)k * ld + row;
        r[it][0] = *(const float4*)p;
        r[it][1] = *(const float4*)(p + ld);
      }
    }
  }
}

// registers -> LDS planes [ROWS][TKG_LD] bf16
template <int ROWS, bool KC, bool X3>
VN_DEV void tk_stash(const float4 (&r)[ROWS / 64][2], bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int tid) {
#pragma unroll
  for (int it = 0; it < ROWS / 64; ++it) {
    const int idx = tid + it * 256;
    const float4 a = r[it][0], b = r[it][1];
    if (KC) {
      uint4 h, l = make_uint4(0u, 0u, 0u, 0u);
      tk_split2<X3>(a.x, a.y, h.x, l.x);
      tk_split2<X3>(a.z, a.w, h.y, l.y);
      tk_split2<X3>(b.x, b.y, h.z, l.z);
      tk_split2<X3>(b.z, b.w, h.w, l.w);
      const int off = (idx >> 2) * TKG_LD + (idx & 3) * 8;
      *(uint4*)(hi + off) = h;
      if (X3) *(uint4*)(lo + off) = l;
    } else {
      const int kp = idx & 15, row = (idx >> 4) * 4;
      uint32_t h[4], l[4] = {0u, 0u, 0u, 0u};
      tk_split2<X3>(a.x, b.x, h[0], l[0]);
      tk_split2<X3>(a.y, b.y, h[1], l[1]);
      tk_split2<X3>(a.z, b.z, h[2], l[2]);
      tk_split2<X3>(a.w, b.w, h[3], l[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ((uint32_t*)(hi + (row + j) * TKG_LD))[kp] = h[j];
        if (X3) ((uint32_t*)(lo + (row + j) * TKG_LD))[kp] = l[j];
      }
    }
  }
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------------
// C[M][N] = sum_k A(m,k) B(k,n) with epilogue; AK / BK / kchunk / blockIdx.z as in tf_gemm.  K % 16 == 0, M % 4 == 0, N % 4 == 0,
// 16-byte aligned rows.
template <int MODE, int WM, bool AK, bool BK, int EPI>
__global__ __launch_bounds__(256) VN_NO_PK_F32 void tk_gemm_bf16(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                                                 float* __restrict__ Cm, int ldc, int M, int N, int K, int kchunk, GemmEpi ep) {
  constexpr bool X3 = MODE == TKM_BF16X3;
  constexpr int BM = 64 * WM, NP = X3 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) bf16_t As[2][NP][BM * TKG_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[2][NP][TKG_BN * TKG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * TKG_BN;
  const int kbeg = blockIdx.z * kchunk, kend = kbeg + kchunk < K ? kbeg + kchunk : K;
  Cm += (long)blockIdx.z * M * ldc;
  f32x4_v acc[WM][4];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_v{0.f, 0.f, 0.f, 0.f};

  float4 ra[WM][2], rb[1][2];
  tk_fetch<BM, AK>(ra, A, lda, m0, M, kbeg, kend, tid);
  tk_fetch<TKG_BN, BK>(rb, Bm, ldb, n0, N, kbeg, kend, tid);
  tk_stash<BM, AK, X3>(ra, As[0][0], As[0][NP - 1], tid);
  tk_stash<TKG_BN, BK, X3>(rb, Bs[0][0], Bs[0][NP - 1], tid);
  __syncthreads();

  const int frag = (lane & 15) * TKG_LD + (lane >> 4) * 8;
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += TKG_BK, buf ^= 1) {
    const bool more = k0 + TKG_BK < kend;
    if (more) {
      tk_fetch<BM, AK>(ra, A, lda, m0, M, k0 + TKG_BK, kend, tid);
      tk_fetch<TKG_BN, BK>(rb, Bm, ldb, n0, N, k0 + TKG_BK, kend, tid);
    }
    bf16x8_v ah[WM], bh[4], al[WM], bl[4];
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int off = (wv * WM + i) * 16 * TKG_LD + frag;
      ah[i] = *(const bf16x8_v*)(As[buf][0] + off);
      if (X3) al[i] = *(const bf16x8_v*)(As[buf][NP - 1] + off);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int off = j * 16 * TKG_LD + frag;
      bh[j] = *(const bf16x8_v*)(Bs[buf][0] + off);
      if (X3) bl[j] = *(const bf16x8_v*)(Bs[buf][NP - 1] + off);
    }
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        if (X3) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
        }
      }
    }
    if (more) {
      tk_stash<BM, AK, X3>(ra, As[buf ^ 1][0], As[buf ^ 1][NP - 1], tid);
      tk_stash<TKG_BN, BK, X3>(rb, Bs[buf ^ 1][0], Bs[buf ^ 1][NP - 1], tid);
    }
    __syncthreads();
  }

  DropKey dk;
  dk.thr = 0; dk.k0 = dk.k1 = 0; dk.scale = 1.f;
  if (tk_epi_drops<EPI>()) dk = drop_key(ep.drop, ep.stream);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + j * 16 + (lane & 15);
    if (n >= N) continue;
    const float bias = tk_epi_bias<EPI>() ? ep.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + (wv * WM + i) * 16 + 4 * (lane >> 4) + r;
        if (m < M) tk_epilogue<EPI>(acc[i][j][r], m, n, N, Cm, ldc, bias, dk, ep);
      }
    }
  }
}

// C = epilogue(sum_z part[z][m][n]), slices in index order: the sliced weight-gradient form of vinet_token_gemm for every epilogue
template <int EPI>
__global__ __launch_bounds__(256) void tk_reduce_epi(const float* __restrict__ part, int nsplit, int M, int N, float* __restrict__ Cm, int ldc, GemmEpi ep) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x, n_el = (long)M * N;
  if (i >= n_el) return;
  const int m = (int)(i / N), n = (int)(i - (long)m * N);
  float s = 0.f;
  for (int z = 0; z < nsplit; ++z) s += part[(long)z * n_el + i];
  DropKey dk;
  dk.thr = 0; dk.k0 = dk.k1 = 0; dk.scale = 1.f;
  if (tk_epi_drops<EPI>()) dk = drop_key(ep.drop, ep.stream);
  tk_epilogue<EPI>(s, m, n, N, Cm, ldc, tk_epi_bias<EPI>() ? ep.bias[n] : 0.f, dk, ep);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
template <int MODE, bool AK, bool BK, int EPI>
static void tk_gemm_bf16_launch(hipStream_t s, const float* A, int lda, const float* Bm, int ldb, float* Cm, int ldc, int M, int N, int K, int kchunk,
                                int nz, const GemmEpi& ep) {
  // 64-row tiles keep every CU busy at a few clips (and serve M = 4); 128 rows reuse a weight fragment for twice the MFMAs
  if (M >= TKG_TALL_M) {
    hipLaunchKernelGGL((tk_gemm_bf16<MODE, 2, AK, BK, EPI>), dim3(vn_div_up(N, TKG_BN), vn_div_up(M, 128), nz), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc,
                       M, N, K, kchunk, ep);
  } else {
    hipLaunchKernelGGL((tk_gemm_bf16<MODE, 1, AK, BK, EPI>), dim3(vn_div_up(N, TKG_BN), vn_div_up(M, 64), nz), dim3(256), 0, s, A, lda, Bm, ldb, Cm, ldc,
                       M, N, K, kchunk, ep);
  }
}

// one product in the arithmetic `mma`: VINET_TK_MMA_F32 is tf_gemm_launch, launch for launch
template <bool AK, bool BK, int EPI>
static void tk_gemm_launch(int mma, hipStream_t s, const float* A, int lda, const float* Bm, int ldb, float* Cm, int ldc, int M, int N, int K,
                           const GemmEpi& ep) {
  if (mma == TKM_F32) tf_gemm_launch<AK, BK, EPI>(s, A, lda, Bm, ldb, Cm, ldc, M, N, K, ep);
  else if (mma == TKM_BF16X3) tk_gemm_bf16_launch<TKM_BF16X3, AK, BK, EPI>(s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, 1, ep);
  else tk_gemm_bf16_launch<TKM_BF16, AK, BK, EPI>(s, A, lda, Bm, ldb, Cm, ldc, M, N, K, K, 1, ep);
}

// the partial matrices of a sliced weight gradient: part[z] = (dY^T X) over rows [z TF_WGRAD_CHUNK, +TF_WGRAD_CHUNK)
static void tk_wgrad_slices(int mma, hipStream_t s, int nsplit, float* part, const float* dY, int ldy, const float* X, int ldx, int rows, int cols, int M) {
  GemmEpi ep;
  memset(&ep, 0, sizeof(ep));
  if (mma == TKM_F32) {
    hipLaunchKernelGGL((tf_gemm<2, false, false, EPI_PLAIN>), dim3(vn_div_up(cols, 64), vn_div_up(rows, 32), nsplit), dim3(256), 0, s, dY, ldy, X, ldx,
                       part, cols, rows, cols, M, TF_WGRAD_CHUNK, ep);
  } else if (mma == TKM_BF16X3) {
    tk_gemm_bf16_launch<TKM_BF16X3, false, false, EPI_PLAIN>(s, dY, ldy, X, ldx, part, cols, rows, cols, M, TF_WGRAD_CHUNK, nsplit, ep);
  } else {
    tk_gemm_bf16_launch<TKM_BF16, false, false, EPI_PLAIN>(s, dY, ldy, X, ldx, part, cols, rows, cols, M, TF_WGRAD_CHUNK, nsplit, ep);
  }
}

// dW[rows][cols] += dY^T X over all M tokens in the arithmetic `mma` (tf_wgrad_launch's scheme; VINET_TK_MMA_F32 is tf_wgrad_launch)
static void tk_wgrad_launch(int mma, hipStream_t s, int nsplit, float* part, const float* dY, int ldy, const float* X, int ldx, float* dW, int rows,
                            int cols, int M) {
  if (mma == TKM_F32) { tf_wgrad_launch(s, nsplit, part, dY, ldy, X, ldx, dW, rows, cols, M); return; }
  if (nsplit <= 1) {
    GemmEpi ep;
    memset(&ep, 0, sizeof(ep));
    tk_gemm_launch<false, false, EPI_ACCUM>(mma, s, dY, ldy, X, ldx, dW, cols, rows, cols, M, ep);
    return;
  }
  tk_wgrad_slices(mma, s, nsplit, part, dY, ldy, X, ldx, rows, cols, M);
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(tf_reduce_split, dim3(vn_div_up(n, 256)), dim3(256), 0, s, part, nsplit, n, dW);
}

}  // namespace
