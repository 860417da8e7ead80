// The max-pool backward gather on the EXEC mask, shared by the block backward kernels of pool.hip and by the BatchNorm-backward
// kernels of bn.hip that form the gradient behind a 1x3x3 / s(1,2,2) / p(0,1,1) pool in registers (bn_bwd_*_pool_kernel).
#pragma once
#include "elementwise.h"

// g += v in the lanes whose code byte (byte BYTE of `word`) equals `code`: v_cmpx (SDWA byte select) -> add under EXEC -> EXEC restored
#define POOL_ADD_IF_X(g, word, BYTE, code, v, exec0)                                                                                  \
  asm volatile("v_cmpx_eq_u32_sdwa vcc, %1, %2 src0_sel:BYTE_" #BYTE " src1_sel:DWORD\n\tv_add_f32_e32 %0, %0, %3\n\ts_mov_b64 exec, %4" \
               : "+v"(g) : "v"(word), "s"(code), "v"(v), "s"(exec0) : "vcc")
#define POOL_ADD_IF(g, word, BYTE, code, v) POOL_ADD_IF_X(g, word, BYTE, code, v, exec0)
// byte e (0..7) of a 64-bit code word
#define POOL_ADD_IF8(g, lo, hi, e, code, v, ex)                                           \
  do {                                                                                      \
    const uint32_t w_ = (e) < 4 ? (lo) : (hi);                                              \
    switch ((e) & 3) {                                                                      \
      case 0: POOL_ADD_IF_X(g, w_, 0, code, v, ex); break;                                  \
      case 1: POOL_ADD_IF_X(g, w_, 1, code, v, ex); break;                                  \
      case 2: POOL_ADD_IF_X(g, w_, 2, code, v, ex); break;                                  \
      default: POOL_ADD_IF_X(g, w_, 3, code, v, ex); break;                                 \
    }                                                                                       \
  } while (0)

// the same with v still a packed bf16 pair: half HALF (0 / 1) of `pair` is widened inside the narrowed EXEC region (one more VALU
// per add, and the 8 gradients of a window stay in 4 registers instead of 8: the BatchNorm kernels of bn.hip have none to spare).
// The add is the same v_add_f32 of the same value.
#define POOL_ADD_IF_PK_X(g, word, BYTE, code, pair, WIDEN, exec0)                                                          \
  do {                                                                                                                     \
    float t_;                                                                                                              \
    asm volatile("v_cmpx_eq_u32_sdwa vcc, %2, %3 src0_sel:BYTE_" #BYTE " src1_sel:DWORD\n\t" WIDEN                         \
                 "\n\tv_add_f32_e32 %0, %0, %1\n\ts_mov_b64 exec, %5"                                                      \
                 : "+v"(g), "=&v"(t_) : "v"(word), "s"(code), "v"(pair), "s"(exec0) : "vcc");                              \
  } while (0)
#define POOL_WIDEN_LO "v_lshlrev_b32_e32 %1, 16, %4"
#define POOL_WIDEN_HI "v_and_b32_e32 %1, 0xffff0000, %4"
#define POOL_ADD_IF8_PK(g, lo, hi, e, code, pair, ex)                                                  \
  do {                                                                                                 \
    const uint32_t w_ = (e) < 4 ? (lo) : (hi);                                                         \
    switch ((e) & 3) {                                                                                 \
      case 0: POOL_ADD_IF_PK_X(g, w_, 0, code, pair, POOL_WIDEN_LO, ex); break;                        \
      case 1: POOL_ADD_IF_PK_X(g, w_, 1, code, pair, POOL_WIDEN_HI, ex); break;                        \
      case 2: POOL_ADD_IF_PK_X(g, w_, 2, code, pair, POOL_WIDEN_LO, ex); break;                        \
      default: POOL_ADD_IF_PK_X(g, w_, 3, code, pair, POOL_WIDEN_HI, ex); break;                       \
    }                                                                                                  \
  } while (0)

// ---- 1x3x3 / s(1,2,2) / p(0,1,1): the 2 x 2 input block (hb, wb) = {2hb, 2hb+1} x {2wb, 2wb+1} x 8 channels of group g ----
// Only the four windows q = dh*2 + dw at (hb + dh, wb + dw) reach it: (hb, wb) all four inputs, (hb, wb+1) and (hb+1, wb) two
// each, (hb+1, wb+1) one.

// the argmax words of the four windows (a window past the edge: ~0, which equals no tap code) and whether each exists
VN_DEV void pool_k133s2_codes(const TView& dy, const uint8_t* __restrict__ argmax, int b, int t, int hb, int wb, int g,
                              unsigned long long am[4], bool wok[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ho = hb + (q >> 1), wo = wb + (q & 1);
    wok[q] = ho < dy.H && wo < dy.W;
    const long ovox = (((long)b * dy.T + t) * dy.H + (wok[q] ? ho : 0)) * dy.W + (wok[q] ? wo : 0);
    am[q] = wok[q] ? *(const unsigned long long*)(argmax + ovox * dy.C + g * 8) : ~0ull;
  }
}

// does any of the 8 channels of window q pick a tap inside the block (rows kh in {1,2} for dh = 0 or {0} for dh = 1; same for columns)
VN_DEV bool pool_k133s2_any(unsigned long long amq, int q) {
  bool any = false;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const bool in = ((q >> 1) ? kh == 0 : kh >= 1) && ((q & 1) ? kw == 0 : kw >= 1);
      if (!in) continue;
      const unsigned long long x = amq ^ ((unsigned long long)(kh * 3 + kw) * 0x0101010101010101ull);
      any |= ((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull) != 0;
    }
  return any;
}

// gr[e] += the gradients dv[q][e] of the windows q = 0...3, in that order, whose argmax is input (ih, iw) of the block (ih, iw:
// compile-time after unrolling).  `ex`: the EXEC mask of the calling region, read there (s_mov_b64 from exec) -- every add restores it.
VN_DEV void pool_k133s2_sum(const unsigned long long am[4], const float dv[4][8], int ih, int iw, unsigned long long ex, float gr[8]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dh = q >> 1, dw = q & 1;
    // input (h, w) as tap (kh, kw) of window (hb + dh, wb + dw): kh = h + 1 - 2*(hb + dh) = ih + 1 - 2*dh
    const int kh = ih + 1 - 2 * dh, kw = iw + 1 - 2 * dw;
    if (kh < 0 || kw < 0) continue;                       // (compile-time: the window does not reach this input)
    const uint32_t alo = (uint32_t)am[q], ahi = (uint32_t)(am[q] >> 32);
#pragma unroll
    for (int e = 0; e < 8; ++e) POOL_ADD_IF8(gr[e], alo, ahi, e, (uint32_t)(kh * 3 + kw), dv[q][e], ex);
  }
}
// the same over packed bf16 rows (dr[q]: the 8 gradients of window q as four pairs)
VN_DEV void pool_k133s2_sum_pk(const unsigned long long am[4], const uint4 dr[4], int ih, int iw, unsigned long long ex, float gr[8]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dh = q >> 1, dw = q & 1;
    const int kh = ih + 1 - 2 * dh, kw = iw + 1 - 2 * dw;
    if (kh < 0 || kw < 0) continue;
    const uint32_t alo = (uint32_t)am[q], ahi = (uint32_t)(am[q] >> 32);
    const uint32_t pw[4] = {dr[q].x, dr[q].y, dr[q].z, dr[q].w};
#pragma unroll
    for (int e = 0; e < 8; ++e) POOL_ADD_IF8_PK(gr[e], alo, ahi, e, (uint32_t)(kh * 3 + kw), pw[e >> 1], ex);
  }
}
