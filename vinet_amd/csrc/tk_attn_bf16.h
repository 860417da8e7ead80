// The token encoder's attention on the bf16 MFMA (v_mfma_f32_16x16x32_bf16): the three kernels of token_encoder.hip (forward, dQ,
// dK / dV) over the same fp32 workspace matrices -- qkv, the saved softmax rows P, ao, dqkv, dot -- with every operand of the seven
// products rounded to bf16 where the fp32 kernel forms it in fp32.
//
// Arithmetic (template parameter MODE, VINET_TK_MMA_BF16 / _BF16X3, the split of tk_gemm_bf16.h: hi = bf16(a), lo = bf16(a - hi)):
//   product             A operand                         B operand   k axis
//   scores = A B^T      q qscale (scaled, then split)     k           D
//   AO     = A B        p m  (softmax value x keep mask)  v           keys
//   dP     = A B^T      dAO                               v           D
//   dQ     = A B        dS                                k           keys
//   dV     = A^T B      P m                               dAO         queries
//   dK     = A^T B      dS                                q           queries
// BF16 sums hi hi, BF16X3 sums hi hi + hi lo + lo hi, fp32 accumulation inside the MFMA.  The row maximum, expf, the row sum, the
// normalisation, the keep-mask draw (same element index), dS = P (dP m - dot) qscale, tk_attn_dot and the values saved in P are the
// fp32 kernels' own statements: a step's masks do not depend on the mode.
//
// Structure: the fp32 family's.  One workgroup per (clip, head, 64 rows), 16 rows per wave; the other side streams through LDS in
// tiles (64 keys forward, 32 backward), converted WHILE it is staged into a hi and a lo plane of bf16:
//   row-major planes   [tile row][32 KS + 8]   the operand whose k axis is D: a lane's fragment is one 16-byte read (8 d at 8 g of
//                                              row n); D is padded with zeros to the MFMA's step of 32
//   transposed planes  [16 DT][tile + 8]       the operand whose k axis is the tile's rows (V in AO, K in dQ, dAO / Q in dV / dK):
//                                              a lane loads four d of two consecutive rows and writes four (row, row + 1) pairs,
//                                              as tk_stash does; d from D to 16 DT is zero
// (row strides of 20, 36, 52, 68 dwords put the 16 rows of a lane group on 16 different 16-byte bank slots.)
// The wave's own rows (q qscale, dAO, v) are split once into registers.  P m and dS leave the MFMA with the column on the lane and
// go through one per-wave LDS tile [16][tile + 8] (hi and lo) to become the next product's A operand.  The dK / dV kernel takes
// dP with QUERIES as the result rows (A = the staged dAO rows, B = the wave's v fragments), so a lane group reads 16 consecutive
// floats of a P row, and writes the hand-off tile transposed, four queries of one key per 8-byte store.
// Rows past a clip's last token are staged as copies of it and masked; padding rows get zeros.  No atomics; each output row is
// summed by one wave in tile order.
//
// The kernels carry VN_NO_PK_F32 (common.h): they form a - hi(a).
#pragma once
#include "tk_gemm_bf16.h"

namespace {

constexpr int TKA_BQ = 64;     // rows per workgroup: 16 per wave
constexpr int TKA_FK = 64;     // keys per LDS tile, forward
constexpr int TKA_BT = 32;     // keys (dQ kernel) / queries (dK / dV kernel) per LDS tile, backward

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_v;

template <bool X3>
VN_DEV void tka_split8(const float4& a, const float4& b, uint4& h, uint4& l) {
  l = make_uint4(0u, 0u, 0u, 0u);
  tk_split2<X3>(a.x, a.y, h.x, l.x);
  tk_split2<X3>(a.z, a.w, h.y, l.y);
  tk_split2<X3>(b.x, b.y, h.z, l.z);
  tk_split2<X3>(b.z, b.w, h.w, l.w);
}

// the wave's own operand: elements [32 ks + 8 g, + 8) of `row` (D floats, zero from D on) times `scale`, split into registers
template <int KS, bool X3>
VN_DEV void tka_row_frags(const float* __restrict__ row, int D, int g, float scale, bf16x8_v (&hi)[KS], bf16x8_v (&lo)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = ks * 32 + 8 * g;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (d0 < D) a = *(const float4*)(row + d0);
    if (d0 + 4 < D) b = *(const float4*)(row + d0 + 4);
    a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
    b.x *= scale; b.y *= scale; b.z *= scale; b.w *= scale;
    uint4 h, l;
    tka_split8<X3>(a, b, h, l);
    hi[ks] = __builtin_bit_cast(bf16x8_v, u32x4_v{h.x, h.y, h.z, h.w});
    lo[ks] = __builtin_bit_cast(bf16x8_v, u32x4_v{l.x, l.y, l.z, l.w});
  }
}

// `rows` rows of D floats from src + row lds -> planes [rows][ld] bf16, Dp = ld - 8 columns (zero from D on); rows past the clip's
// last token repeat it (finite, masked by the caller)
template <bool X3>
VN_DEV void tka_stage_rows(bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int ld, const float* __restrict__ src, long lds, int row0, int rows,
                           int S, int D) {
  const int n8 = (ld - 8) >> 3;
  for (int idx = threadIdx.x; idx < rows * n8; idx += 256) {
    const int r = idx / n8, c = (idx - r * n8) * 8;
    const int row = row0 + r < S ? row0 + r : S - 1;
    const float* p = src + (long)row * lds + c;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (c < D) a = *(const float4*)p;
    if (c + 4 < D) b = *(const float4*)(p + 4);
    uint4 h, l;
    tka_split8<X3>(a, b, h, l);
    *(uint4*)(hi + r * ld + c) = h;
    if (X3) *(uint4*)(lo + r * ld + c) = l;
  }
}

// T rows of D floats -> transposed planes [4 nq][T + 8] bf16 (column d of the source = row d of the plane; zero from D on)
template <int T, bool X3>
VN_DEV void tka_stage_cols(bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, const float* __restrict__ src, long lds, int row0, int S, int D, int nq) {
  constexpr int HP = T / 2, LDT = T + 8;
  for (int idx = threadIdx.x; idx < HP * nq; idx += 256) {
    const int kp = idx % HP, d = (idx / HP) * 4;
    const int r0 = row0 + 2 * kp < S ? row0 + 2 * kp : S - 1, r1 = row0 + 2 * kp + 1 < S ? row0 + 2 * kp + 1 : S - 1;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (d < D) {
      a = *(const float4*)(src + (long)r0 * lds + d);
      b = *(const float4*)(src + (long)r1 * lds + d);
    }
    uint32_t h[4], l[4] = {0u, 0u, 0u, 0u};
    tk_split2<X3>(a.x, b.x, h[0], l[0]);
    tk_split2<X3>(a.y, b.y, h[1], l[1]);
    tk_split2<X3>(a.z, b.z, h[2], l[2]);
    tk_split2<X3>(a.w, b.w, h[3], l[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ((uint32_t*)(hi + (d + j) * LDT))[kp] = h[j];
      if (X3) ((uint32_t*)(lo + (d + j) * LDT))[kp] = l[j];
    }
  }
}

// acc += A B in the mode's terms
template <bool X3>
VN_DEV void tka_mma(f32x4_v& acc, const bf16x8_v& ah, const bf16x8_v& al, const bf16_t* __restrict__ bhi, const bf16_t* __restrict__ blo, int off) {
  const bf16x8_v bh = *(const bf16x8_v*)(bhi + off);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
  if (X3) {
    const bf16x8_v bl = *(const bf16x8_v*)(blo + off);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// DT = 16-column tiles of the head width (D <= 16 DT, D % 4 == 0); KS = 32-wide k-steps over D.
template <int MODE, int DT>
__global__ __launch_bounds__(256) VN_NO_PK_F32 void tk_attn_fwd_bf16(const float* __restrict__ qkv, int S, int Sp, int E, int H, int D, float qscale,
                                                                     float* P, float* __restrict__ ao, Drop drop, int stream,
                                                                     uint8_t* __restrict__ mask) {
  constexpr bool X3 = MODE == TKM_BF16X3;
  constexpr int NP = X3 ? 2 : 1, KS = (DT + 1) / 2, LDR = KS * 32 + 8, LDT = TKA_FK + 8;
  constexpr int TILE = TKA_FK * LDR > 16 * DT * LDT ? TKA_FK * LDR : 16 * DT * LDT;     // K row-major, then V transposed
  __shared__ __attribute__((aligned(16))) bf16_t kv[NP][TILE];
  __shared__ __attribute__((aligned(16))) bf16_t ps[NP][4][16 * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const float* base = qkv + (long)b * Sp * 3 * E + h * D;
  const int q0 = blockIdx.x * TKA_BQ + wv * 16;
  const long prow0 = ((long)b * H + h) * S;
  const int qrow = q0 + n < S ? q0 + n : S - 1;
  bf16x8_v qh[KS], ql[KS];
  tka_row_frags<KS, X3>(base + (long)qrow * 3 * E, D, g, qscale, qh, ql);

  // pass 1: raw scores into P, running maximum and sum of each row over this lane's columns
  float mx[4], sm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { mx[r] = -INFINITY; sm[r] = 0.f; }
  for (int k0 = 0; k0 < S; k0 += TKA_FK) {
    __syncthreads();
    tka_stage_rows<X3>(kv[0], kv[NP - 1], LDR, base + E, 3 * E, k0, TKA_FK, S, D);
    __syncthreads();
#pragma unroll 1
    for (int nt = 0; nt < TKA_FK / 16; ++nt) {
      f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) tka_mma<X3>(acc, qh[ks], ql[ks], kv[0], kv[NP - 1], (nt * 16 + n) * LDR + ks * 32 + 8 * g);
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

  // pass 2: normalise (P keeps the softmax rows), dropout, O = (P m) V
  const DropKey dk = drop_key(drop, stream);
  f32x4_v o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += TKA_FK) {
    __syncthreads();
    tka_stage_cols<TKA_FK, X3>(kv[0], kv[NP - 1], base + 2 * E, 3 * E, k0, S, D, 4 * DT);
#pragma unroll
    for (int nt = 0; nt < TKA_FK / 16; ++nt) {
      const int j = k0 + nt * 16 + n;
      float pv[4];
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
        pv[r] = p;
      }
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        uint32_t hh, ll = 0u;
        tk_split2<X3>(pv[r], pv[r + 1], hh, ll);
        const int off = (4 * g + r) * LDT + nt * 16 + n;
        ps[0][wv][off] = (bf16_t)hh;
        ps[0][wv][off + LDT] = (bf16_t)(hh >> 16);
        if (X3) {
          ps[NP - 1][wv][off] = (bf16_t)ll;
          ps[NP - 1][wv][off + LDT] = (bf16_t)(ll >> 16);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < TKA_FK / 32; ++ks) {
      if (k0 + ks * 32 < S) {      // (a k-step past the last key holds zeros only)
        const int offa = n * LDT + ks * 32 + 8 * g;
        const bf16x8_v ah = *(const bf16x8_v*)(ps[0][wv] + offa);
        bf16x8_v al = ah;
        if (X3) al = *(const bf16x8_v*)(ps[NP - 1][wv] + offa);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          if (dt * 16 < D) tka_mma<X3>(o[dt], ah, al, kv[0], kv[NP - 1], (dt * 16 + n) * LDT + ks * 32 + 8 * g);
      }
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

// ---- dQ: one wave per 16 queries, keys in tiles of TKA_BT.  dS = P (dP m - dot) qscale with dP = dAO V^T ------------------------
template <int MODE, int DT>
__global__ __launch_bounds__(256) VN_NO_PK_F32 void tk_attn_bwd_q_bf16(const float* __restrict__ qkv, const float* __restrict__ P,
                                                                       const float* __restrict__ dao, const float* __restrict__ dot, int S, int Sp, int E,
                                                                       int H, int D, float qscale, float* __restrict__ dqkv, Drop drop, int stream) {
  constexpr bool X3 = MODE == TKM_BF16X3;
  constexpr int NP = X3 ? 2 : 1, KS = (DT + 1) / 2, LDR = KS * 32 + 8, LDT = TKA_BT + 8;
  __shared__ __attribute__((aligned(16))) bf16_t vr[NP][TKA_BT * LDR];      // V, row-major
  __shared__ __attribute__((aligned(16))) bf16_t kc[NP][16 * DT * LDT];     // K, transposed
  __shared__ __attribute__((aligned(16))) bf16_t ps[NP][4][16 * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const float* base = qkv + (long)b * Sp * 3 * E + h * D;
  const int q0 = blockIdx.x * TKA_BQ + wv * 16;
  const long prow0 = ((long)b * H + h) * S;
  const int qrow = q0 + n < S ? q0 + n : S - 1;
  bf16x8_v gh[KS], gl[KS];
  tka_row_frags<KS, X3>(dao + ((long)b * Sp + qrow) * E + h * D, D, g, 1.f, gh, gl);
  float dotr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 4 * g + r;
    dotr[r] = dot[((long)b * Sp + (i < S ? i : S - 1)) * H + h];
  }
  const DropKey dk = drop_key(drop, stream);
  f32x4_v dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += TKA_BT) {
    __syncthreads();
    tka_stage_rows<X3>(vr[0], vr[NP - 1], LDR, base + 2 * E, 3 * E, k0, TKA_BT, S, D);
    tka_stage_cols<TKA_BT, X3>(kc[0], kc[NP - 1], base + E, 3 * E, k0, S, D, 4 * DT);
    __syncthreads();
#pragma unroll 1
    for (int nt = 0; nt < TKA_BT / 16; ++nt) {
      f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) tka_mma<X3>(acc, gh[ks], gl[ks], vr[0], vr[NP - 1], (nt * 16 + n) * LDR + ks * 32 + 8 * g);
      const int j = k0 + nt * 16 + n;
      float sv[4];
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
        sv[r] = ds;
      }
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        uint32_t hh, ll = 0u;
        tk_split2<X3>(sv[r], sv[r + 1], hh, ll);
        const int off = (4 * g + r) * LDT + nt * 16 + n;
        ps[0][wv][off] = (bf16_t)hh;
        ps[0][wv][off + LDT] = (bf16_t)(hh >> 16);
        if (X3) {
          ps[NP - 1][wv][off] = (bf16_t)ll;
          ps[NP - 1][wv][off + LDT] = (bf16_t)(ll >> 16);
        }
      }
    }
    __syncthreads();
    const int offa = n * LDT + 8 * g;
    const bf16x8_v ah = *(const bf16x8_v*)(ps[0][wv] + offa);
    bf16x8_v al = ah;
    if (X3) al = *(const bf16x8_v*)(ps[NP - 1][wv] + offa);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      if (dt * 16 < D) tka_mma<X3>(dq[dt], ah, al, kc[0], kc[NP - 1], (dt * 16 + n) * LDT + 8 * g);
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

// ---- dK, dV: one wave per 16 keys, queries in tiles of TKA_BT.  dP = dAO V^T with the tile's queries as result rows and the wave's
// keys on the lanes; (P m)^T and dS^T go through the hand-off tiles [key][query]; dV += (P m)^T dAO and dK += dS^T Q -----------------
template <int MODE, int DT>
__global__ __launch_bounds__(256) VN_NO_PK_F32 void tk_attn_bwd_kv_bf16(const float* __restrict__ qkv, const float* __restrict__ P,
                                                                        const float* __restrict__ dao, const float* __restrict__ dot, int S, int Sp, int E,
                                                                        int H, int D, float qscale, float* __restrict__ dqkv, Drop drop, int stream) {
  constexpr bool X3 = MODE == TKM_BF16X3;
  constexpr int NP = X3 ? 2 : 1, KS = (DT + 1) / 2, LDR = KS * 32 + 8, LDT = TKA_BT + 8;
  // one buffer, two uses per tile (the block stays below 64 KB at D = 128): first dAO row-major for dP, then dAO and Q transposed
  constexpr int TP = 16 * DT * LDT;
  static_assert(TKA_BT * LDR <= 2 * TP, "the row-major tile must fit the two transposed ones");
  __shared__ __attribute__((aligned(16))) bf16_t tile[NP][2 * TP];
  bf16_t *const gr0 = tile[0], *const gr1 = tile[NP - 1];               // dAO, row-major
  bf16_t *const gc0 = tile[0], *const gc1 = tile[NP - 1];               // dAO, transposed
  bf16_t *const qc0 = tile[0] + TP, *const qc1 = tile[NP - 1] + TP;     // Q, transposed
  __shared__ __attribute__((aligned(16))) bf16_t pt[NP][4][16 * LDT], st[NP][4][16 * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const float* base = qkv + (long)b * Sp * 3 * E + h * D;
  const float* gbase = dao + (long)b * Sp * E + h * D;
  const int j0 = blockIdx.x * TKA_BQ + wv * 16;
  const long prow0 = ((long)b * H + h) * S;
  const int krow = j0 + n < S ? j0 + n : S - 1;
  bf16x8_v vh[KS], vl[KS];
  tka_row_frags<KS, X3>(base + (long)krow * 3 * E + 2 * E, D, g, 1.f, vh, vl);
  const DropKey dk = drop_key(drop, stream);
  f32x4_v dv[DT], dkk[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) { dv[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f}; dkk[dt] = f32x4_v{0.f, 0.f, 0.f, 0.f}; }
  for (int i0 = 0; i0 < S; i0 += TKA_BT) {
    __syncthreads();
    tka_stage_rows<X3>(gr0, gr1, LDR, gbase, E, i0, TKA_BT, S, D);
    __syncthreads();
    const int j = j0 + n;
#pragma unroll 1
    for (int nt = 0; nt < TKA_BT / 16; ++nt) {
      f32x4_v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        // (A = the staged dAO rows, B = the wave's v: the three terms are hi hi + lo hi + hi lo, the same set)
        const int off = (nt * 16 + n) * LDR + ks * 32 + 8 * g;
        const bf16x8_v ah = *(const bf16x8_v*)(gr0 + off);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, vh[ks], acc, 0, 0, 0);
        if (X3) {
          const bf16x8_v al = *(const bf16x8_v*)(gr1 + off);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, vl[ks], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, vh[ks], acc, 0, 0, 0);
        }
      }
      float pv[4], sv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + nt * 16 + 4 * g + r;
        float pd = 0.f, ds = 0.f;
        if (i < S && j < S) {
          const float dt_i = dot[((long)b * Sp + i) * H + h];
          const long e = (prow0 + i) * S + j;
          float m = 1.f;
          if (dk.thr) m = drop_keep(dk, (uint32_t)e) ? dk.scale : 0.f;
          const float p = P[e];
          pd = p * m;
          ds = p * (acc[r] * m - dt_i) * qscale;
        }
        pv[r] = pd;
        sv[r] = ds;
      }
      uint2 ph, pl = make_uint2(0u, 0u), sh, sl = make_uint2(0u, 0u);
      tk_split2<X3>(pv[0], pv[1], ph.x, pl.x);
      tk_split2<X3>(pv[2], pv[3], ph.y, pl.y);
      tk_split2<X3>(sv[0], sv[1], sh.x, sl.x);
      tk_split2<X3>(sv[2], sv[3], sh.y, sl.y);
      const int off = n * LDT + nt * 16 + 4 * g;
      *(uint2*)(pt[0][wv] + off) = ph;
      *(uint2*)(st[0][wv] + off) = sh;
      if (X3) {
        *(uint2*)(pt[NP - 1][wv] + off) = pl;
        *(uint2*)(st[NP - 1][wv] + off) = sl;
      }
    }
    __syncthreads();
    tka_stage_cols<TKA_BT, X3>(gc0, gc1, gbase, E, i0, S, D, 4 * DT);
    tka_stage_cols<TKA_BT, X3>(qc0, qc1, base, 3 * E, i0, S, D, 4 * DT);
    __syncthreads();
    const int offa = n * LDT + 8 * g;
    const bf16x8_v a1h = *(const bf16x8_v*)(pt[0][wv] + offa), a2h = *(const bf16x8_v*)(st[0][wv] + offa);
    bf16x8_v a1l = a1h, a2l = a2h;
    if (X3) {
      a1l = *(const bf16x8_v*)(pt[NP - 1][wv] + offa);
      a2l = *(const bf16x8_v*)(st[NP - 1][wv] + offa);
    }
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      if (dt * 16 < D) {
        const int offb = (dt * 16 + n) * LDT + 8 * g;
        tka_mma<X3>(dv[dt], a1h, a1l, gc0, gc1, offb);
        tka_mma<X3>(dkk[dt], a2h, a2l, qc0, qc1, offb);
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

// ---- launchers ----------------------------------------------------------------------------------------------------------------
#define TKA_BY_WIDTH(D, CALL)                \
  do {                                       \
    if ((D) <= 16) { CALL(1); }              \
    else if ((D) <= 32) { CALL(2); }         \
    else if ((D) <= 64) { CALL(4); }         \
    else { CALL(8); }                        \
  } while (0)

template <int MODE>
static void tk_attn_fwd_bf16_mode(hipStream_t s, const float* qkv, int B, int S, int Sp, int E, int H, float qscale, float* P, float* ao, const Drop& drop,
                                  int stream, uint8_t* mask) {
  const dim3 grid(vn_div_up(S, TKA_BQ), H, B);
  const int D = E / H;
#define TKA_FWD(DT) hipLaunchKernelGGL((tk_attn_fwd_bf16<MODE, DT>), grid, dim3(256), 0, s, qkv, S, Sp, E, H, D, qscale, P, ao, drop, stream, mask)
  TKA_BY_WIDTH(D, TKA_FWD);
#undef TKA_FWD
}

template <int MODE>
static void tk_attn_bwd_bf16_mode(hipStream_t s, const float* qkv, const float* P, const float* dao, const float* dot, int B, int S, int Sp, int E, int H,
                                  float qscale, float* dqkv, const Drop& drop, int stream) {
  const dim3 grid(vn_div_up(S, TKA_BQ), H, B);
  const int D = E / H;
#define TKA_BWD(DT)                                                                                                                              \
  hipLaunchKernelGGL((tk_attn_bwd_q_bf16<MODE, DT>), grid, dim3(256), 0, s, qkv, P, dao, dot, S, Sp, E, H, D, qscale, dqkv, drop, stream);     \
  hipLaunchKernelGGL((tk_attn_bwd_kv_bf16<MODE, DT>), grid, dim3(256), 0, s, qkv, P, dao, dot, S, Sp, E, H, D, qscale, dqkv, drop, stream)
  TKA_BY_WIDTH(D, TKA_BWD);
#undef TKA_BWD
}

// attention of one layer in the arithmetic `attn` (VINET_TK_MMA_BF16X3 or _BF16; F32 is the caller's own family)
static void tk_attn_fwd_bf16_launch(int attn, hipStream_t s, const float* qkv, int B, int S, int Sp, int E, int H, float qscale, float* P, float* ao,
                                    const Drop& drop, int stream, uint8_t* mask) {
  if (attn == TKM_BF16X3) tk_attn_fwd_bf16_mode<TKM_BF16X3>(s, qkv, B, S, Sp, E, H, qscale, P, ao, drop, stream, mask);
  else tk_attn_fwd_bf16_mode<TKM_BF16>(s, qkv, B, S, Sp, E, H, qscale, P, ao, drop, stream, mask);
}
static void tk_attn_bwd_bf16_launch(int attn, hipStream_t s, const float* qkv, const float* P, const float* dao, const float* dot, int B, int S, int Sp,
                                    int E, int H, float qscale, float* dqkv, const Drop& drop, int stream) {
  if (attn == TKM_BF16X3) tk_attn_bwd_bf16_mode<TKM_BF16X3>(s, qkv, P, dao, dot, B, S, Sp, E, H, qscale, dqkv, drop, stream);
  else tk_attn_bwd_bf16_mode<TKM_BF16>(s, qkv, P, dao, dot, B, S, Sp, E, H, qscale, dqkv, drop, stream);
}

}  // namespace
