// The decoder tail at full resolution (bf16, gfx950): everything between the last upsample and the loss of the 32- / 48- / 64-frame
// decoders is a per-pixel function of kT x 32 input values,
//
//   u [B, kT*To, H, W, 32] -> conv 32->32 (kT,1,1)/s(kT,1,1) (+bias) -> ReLU -> a6 -> conv 32->1 + bias -> sigmoid -> map [B, H, W]
//
// and runs here as ONE pass forward and ONE pass backward instead of three and seven launches of the general kernels (conv_dma
// twice + the export; the import, vinet_act_bwd twice, conv_pw and one conv_dma per tap), several of which moved an fp32 head
// padded 1 -> 8 channels.
//
// The results are the BITS of those launches, by construction:
//   * the same v_mfma_f32_16x16x32_bf16 products, weights as the A operand (conv_igemm.h: the transposed tile), issued in the same
//     K order (tap-major, the pack's channel order) into accumulators that start at zero.  A voxel's column of an MFMA depends on
//     no other column, so how voxels are grouped into tiles does not matter;
//   * the epilogues' own operations in their order: fmaf(acc, 1, bias) where there is a bias, v_cvt_pk_bf16_f32, ReLU as a signed
//     16-bit max, 1 / (1 + __expf(-v)) behind fmaxf(v, -inf);
//   * backward: dy = bf16(g * (s * (1 - s))) (vinet_act_bwd), the head's data gradient as the MFMA conv_pw issues over the
//     8-channel-padded dy (so that a product of -0 meets the +0 accumulator exactly as there), its bf16 rounding, the ReLU gate
//     `!(a6 > 0) -> +0`, one MFMA K step per tap for du.
//
// Layout.  A wave owns groups of 16 consecutive voxels.  u is loaded straight into the MFMA B-operand layout: lane (p = lane & 15,
// q = lane >> 4) holds channels 8q .. 8q + 7 of voxel p, 16 bytes, so a wave-load covers 1 KB of consecutive memory per tap.  The
// weights (kT x 2 KB + 64 B) live in registers as A fragments.  An accumulator tile arrives as 4 consecutive channels of one voxel
// per lane; a wave-private 1 KB LDS image (16-byte chunk index XOR (row >> 2) & 3: conflict-free both ways) turns it back into
// the 16-bytes-per-lane layout, which is at once the next MFMA's B operand and a whole-row store.  No workgroup barrier anywhere.
#include "conv_igemm.h"
#include "elementwise.h"

namespace {

struct TailArgs {
  const char* u; long u_sB; int u_ld;          // [B, kT*To, H, W, 32] bf16
  char* a6; long a6_sB; int a6_ld;             // [B, To, H, W, 32] bf16 (forward: may be null)
  const char* w_mid;                           // forward: [kT][32 n][32 c]; backward: the transposed pack [kT][32 c][32 n]
  const float* b_mid;                          // or null
  const char* w_head;                          // [32] bf16 (the forward pack of the 32 -> 1 conv)
  const float* b_head;
  float* out; long o_sb, o_sh, o_sw;           // [B, H, W] fp32, any strides (elements)
  const float* g; long g_sb, g_sh, g_sw;       // backward: the map's gradient
  char* dy; long dy_sB; int dy_ld;             // [B, To, H, W, 8] bf16, channel 0 real
  char* dz; long dz_sB; int dz_ld;             // [B, To, H, W, 32] bf16
  char* du; long du_sB; int du_ld;             // [B, kT*To, H, W, 32] bf16
  int To, H, W, HW, M;                         // M = B * To * H * W voxels of a6
  int groups_per_wave;                         // consecutive 16-voxel groups a wave walks
  FastDiv dW, dHW, dTo;
};

// v_cvt_pk_bf16_f32 and v_pk_max_i16 as the compiler's own instructions (what conv_igemm.h / common.h issue from inline asm): they
// read MFMA results here, and only for instructions it knows does the compiler insert the wait states behind an MFMA
typedef __attribute__((ext_vector_type(2))) __bf16 tail_bf16x2_v;
typedef __attribute__((ext_vector_type(2))) short tail_s16x2_v;
VN_DEV uint32_t tail_pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(((f32x2_v){lo, hi}), tail_bf16x2_v));
}
VN_DEV uint32_t tail_pk_relu(uint32_t u) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(tail_s16x2_v, u), ((tail_s16x2_v){0, 0})));
}

constexpr int TAIL_WAVE_LDS = 1024;            // one [16 voxels][32 channels] bf16 image per wave

// the image: lane (p, q) writes its 4 channels of column tile j (8 bytes), then reads channels 8q .. 8q + 7 of voxel p (16 bytes)
VN_DEV void img_put(char* img, int p, int q, int j, uint32_t lo, uint32_t hi) {
  *(uint2*)(img + p * 64 + (((j * 2 + (q >> 1)) ^ ((p >> 2) & 3)) << 4) + (q & 1) * 8) = make_uint2(lo, hi);
}
VN_DEV uint4 img_get(const char* img, int p, int q) { return *(const uint4*)(img + p * 64 + ((q ^ ((p >> 2) & 3)) << 4)); }

struct Vox { int b, to, hw, h, w; };
VN_DEV Vox tail_decode(const TailArgs& a, int m) {
  Vox v;
  const uint32_t bt = fdiv((uint32_t)m, a.dHW);
  v.hw = m - (int)bt * a.HW;
  const uint32_t b = fdiv(bt, a.dTo);
  v.to = (int)bt - (int)b * a.To;
  v.b = (int)b;
  const uint32_t h = fdiv((uint32_t)v.hw, a.dW);
  v.h = (int)h;
  v.w = v.hw - (int)h * a.W;
  return v;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(256, 4) void decoder_tail_fwd_kernel(const TailArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TAIL_WAVE_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  char* img = smem + wave * TAIL_WAVE_LDS;

  // A fragments: row n = 16 j + p of tap t, k = 8q .. 8q + 7; the head's single row lives in the lanes p == 0
  bf16x8_v wm[KT][2];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) wm[t][j] = *(const bf16x8_v*)(a.w_mid + ((long)((t * 32 + j * 16 + p) * 32 + q * 8)) * 2);
  const uint4 wh4 = p == 0 ? *(const uint4*)(a.w_head + q * 16) : make_uint4(0, 0, 0, 0);
  const bf16x8_v wh = __builtin_bit_cast(bf16x8_v, wh4);
  float bm[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) bm[j][r] = a.b_mid ? a.b_mid[j * 16 + q * 4 + r] : 0.f;
  const bool mid_bias = a.b_mid != nullptr;
  const float bh = a.b_head[0];

  // group i + 1's loads are issued before group i is computed: they stay in flight across the image's wave-level fences
  struct Group { Vox v; bool ok; uint4 x[KT]; };
  auto fetch = [&](long m0, Group& g) {
    const int m = (int)m0 + p;
    g.ok = m < a.M;
    g.v = tail_decode(a, g.ok ? m : a.M - 1);      // rows past the end re-read the last voxel (never stored)
    const char* up = a.u + ((long)g.v.b * a.u_sB + ((long)g.v.to * KT * a.HW + g.v.hw) * (long)a.u_ld + q * 8) * 2;
#pragma unroll
    for (int t = 0; t < KT; ++t) g.x[t] = *(const uint4*)(up + (long)t * a.HW * a.u_ld * 2);
  };
  const long g0 = ((long)blockIdx.x * 4 + wave) * a.groups_per_wave;
  Group cur{}, nxt{};
  if (g0 * 16 < a.M) fetch(g0 * 16, cur);
  for (int gi = 0; gi < a.groups_per_wave; ++gi) {
    const long m0 = (g0 + gi) * 16;
    if (m0 >= a.M) break;                      // (wave-uniform)
    const bool more = gi + 1 < a.groups_per_wave && m0 + 16 < a.M;
    if (more) fetch(m0 + 16, nxt);
    const Vox v = cur.v;
    const bool ok = cur.ok;
    uint4 x[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) x[t] = cur.x[t];
    cur = nxt;

    f32x4_v acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      acc[j] = (f32x4_v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < KT; ++t)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm[t][j], __builtin_bit_cast(bf16x8_v, x[t]), acc[j], 0, 0, 0);
    }
    // conv_epilogue's bf16 path: (+bias) -> bf16 -> ReLU, then through the image into the operand / row layout
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float z[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) z[r] = mid_bias ? fmaf(acc[j][r], 1.f, bm[j][r]) : acc[j][r];
      img_put(img, p, q, j, tail_pk_relu(tail_pk_bf16(z[0], z[1])), tail_pk_relu(tail_pk_bf16(z[2], z[3])));
    }
    wave_lds_fence();
    const uint4 a6v = img_get(img, p, q);
    wave_lds_fence();                          // every lane has read the image before the next group overwrites it
    if (a.a6 && ok) st16_nt(a.a6 + ((long)v.b * a.a6_sB + ((long)v.to * a.HW + v.hw) * (long)a.a6_ld + q * 8) * 2, a6v);

    // the head: one K step over a6; row 0 of the tile = lanes q == 0, element 0.  conv_epilogue's general path: affine, sigmoid
    f32x4_v hacc = (f32x4_v){0.f, 0.f, 0.f, 0.f};
    hacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, __builtin_bit_cast(bf16x8_v, a6v), hacc, 0, 0, 0);
    if (q == 0 && ok) {
      float o = fmaxf(fmaf(hacc[0], 1.f, bh), -INFINITY);
      o = 1.f / (1.f + __expf(-o));
      a.out[(long)v.b * a.o_sb + (long)v.h * a.o_sh + (long)v.w * a.o_sw] = o;
    }
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(256, 4) void decoder_tail_bwd_kernel(const TailArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TAIL_WAVE_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = lane & 15, q = lane >> 4;
  char* img = smem + wave * TAIL_WAVE_LDS;

  // A fragments of the data gradients: the transposed pack, row c = 16 j + p (input channel) of tap t, k = output channels
  // 8q .. 8q + 7; the head's transposed pack is [32 c][k = 0: w_head[c], zeros]
  bf16x8_v wt[KT][2];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) wt[t][j] = *(const bf16x8_v*)(a.w_mid + ((long)((t * 32 + j * 16 + p) * 32 + q * 8)) * 2);
  bf16x8_v wh[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t w = q == 0 ? (uint32_t)((const bf16_t*)a.w_head)[j * 16 + p] : 0u;
    wh[j] = __builtin_bit_cast(bf16x8_v, make_uint4(w, 0, 0, 0));
  }

  // group i + 1's loads (a6, and in the lanes q == 0 the map and its gradient) are issued before group i is computed
  struct Group { Vox v; bool ok; uint4 a6v; float g, s; };
  auto fetch = [&](long m0, Group& r) {
    const int m = (int)m0 + p;
    r.ok = m < a.M;
    r.v = tail_decode(a, r.ok ? m : a.M - 1);
    r.a6v = *(const uint4*)(a.a6 + ((long)r.v.b * a.a6_sB + ((long)r.v.to * a.HW + r.v.hw) * (long)a.a6_ld + q * 8) * 2);
    r.g = r.s = 0.f;
    if (q == 0) {
      r.g = a.g[(long)r.v.b * a.g_sb + (long)r.v.h * a.g_sh + (long)r.v.w * a.g_sw];
      r.s = a.out[(long)r.v.b * a.o_sb + (long)r.v.h * a.o_sh + (long)r.v.w * a.o_sw];
    }
  };
  const long g0 = ((long)blockIdx.x * 4 + wave) * a.groups_per_wave;
  Group cur{}, nxt{};
  if (g0 * 16 < a.M) fetch(g0 * 16, cur);
  for (int gi = 0; gi < a.groups_per_wave; ++gi) {
    const long m0 = (g0 + gi) * 16;
    if (m0 >= a.M) break;                      // (wave-uniform)
    const bool more = gi + 1 < a.groups_per_wave && m0 + 16 < a.M;
    if (more) fetch(m0 + 16, nxt);
    const Vox v = cur.v;
    const bool ok = cur.ok;
    const uint4 a6v = cur.a6v;
    const long vox = (long)v.to * a.HW + v.hw;

    // dy = bf16(g * (s * (1 - s))) in channel 0 of the padded head gradient, pad channels zero (vinet_act_bwd over the padded head)
    uint32_t dyb = 0;
    if (q == 0) {
      float gv = cur.g;
      const float s = cur.s;
      gv *= s * (1.f - s);
      dyb = tail_pk_bf16(gv, 0.f) & 0xffffu;
      if (ok) *(uint4*)(a.dy + ((long)v.b * a.dy_sB + vox * (long)a.dy_ld) * 2) = make_uint4(dyb, 0, 0, 0);
    }
    cur = nxt;
    // the head's data gradient: one K step over the padded dy (conv_pw), rounded to bf16
    const bf16x8_v dyf = __builtin_bit_cast(bf16x8_v, make_uint4(dyb, 0, 0, 0));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4_v acc = (f32x4_v){0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], dyf, acc, 0, 0, 0);
      img_put(img, p, q, j, tail_pk_bf16(acc[0], acc[1]), tail_pk_bf16(acc[2], acc[3]));
    }
    wave_lds_fence();
    const uint4 da = img_get(img, p, q);
    wave_lds_fence();
    // ReLU' (vinet_act_bwd): !(a6 > 0) -> +0
    uint4 dzv;
    {
      const uint32_t aw[4] = {a6v.x, a6v.y, a6v.z, a6v.w}, gw[4] = {da.x, da.y, da.z, da.w};
      uint32_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t lo = __uint_as_float(aw[e] << 16) > 0.f ? (gw[e] & 0xffffu) : 0u;
        const uint32_t hi = __uint_as_float(aw[e] & 0xffff0000u) > 0.f ? (gw[e] & 0xffff0000u) : 0u;
        o[e] = lo | hi;
      }
      dzv = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if (ok) *(uint4*)(a.dz + ((long)v.b * a.dz_sB + vox * (long)a.dz_ld + q * 8) * 2) = dzv;

    // du[tap] = dz6 . W_mid[tap]: one K step per tap (the per-tap conv_dma data gradients), stored
    char* dup = a.du + ((long)v.b * a.du_sB + ((long)v.to * KT * a.HW + v.hw) * (long)a.du_ld + q * 8) * 2;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x4_v acc = (f32x4_v){0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[t][j], __builtin_bit_cast(bf16x8_v, dzv), acc, 0, 0, 0);
        img_put(img, p, q, j, tail_pk_bf16(acc[0], acc[1]), tail_pk_bf16(acc[2], acc[3]));
      }
      wave_lds_fence();
      const uint4 d = img_get(img, p, q);
      wave_lds_fence();
      if (ok) st16_nt(dup + (long)t * a.HW * a.du_ld * 2, d);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool tail_view_ok(const VinetTensor* t, int C) { return t && oct_ok(*t) && t->C == C && t->B > 0 && t->T > 0 && t->H > 0 && t->W > 0; }

// what both entry points share: bf16, 32 -> 32 -> 1, (kT,1,1)/s(kT,1,1) with kT in {2,3,4} over a u of exactly kT frames
int tail_common_args(const char* what, int32_t dtype, const VinetTensor* u, int32_t kT, const void* w_mid, const void* w_head,
                     const VinetTensor* a6, bool a6_needed) {
  VN_CHECK_ARG(dtype == VINET_BF16, "%s: bf16 only (dtype %d)", what, dtype);
  VN_CHECK_ARG(kT >= 2 && kT <= 4, "%s: temporal kernel %d not in {2,3,4}", what, kT);
  VN_CHECK_ARG(tail_view_ok(u, 32), "%s: u must be a 32-channel bf16 view on the 16-byte grid", what);
  VN_CHECK_ARG(u->T == kT, "%s: u has %d frames, the temporal kernel %d (one output frame is served)", what, u->T, kT);
  VN_CHECK_ARG(w_mid && w_head && ((uintptr_t)w_mid % 16) == 0 && ((uintptr_t)w_head % 16) == 0, "%s: null or misaligned weight pack", what);
  VN_CHECK_ARG(a6 || !a6_needed, "%s: a6 missing", what);
  if (a6) {
    VN_CHECK_ARG(tail_view_ok(a6, 32), "%s: a6 must be a 32-channel bf16 view on the 16-byte grid", what);
    VN_CHECK_ARG(a6->B == u->B && a6->T * kT == u->T && a6->H == u->H && a6->W == u->W, "%s: a6 is not u's extent at T / %d", what, kT);
  }
  VN_CHECK_ARG((long)u->B * (u->T / kT) * u->H * u->W < (1L << 31) - 16, "%s: too many voxels", what);
  return 0;
}

int tail_fwd_args(const char* what, int32_t dtype, const VinetTensor* u, int32_t kT, const void* w_mid, const float* b_mid,
                  const void* w_head, const float* b_head, const VinetTensor* a6, const float* out) {
  (void)b_mid;
  if (tail_common_args(what, dtype, u, kT, w_mid, w_head, a6, false)) return -1;
  VN_CHECK_ARG(b_head, "%s: the head needs its bias", what);
  VN_CHECK_ARG(out && ((uintptr_t)out % 4) == 0, "%s: null or misaligned map", what);
  return 0;
}

void tail_shape(TailArgs& a, const VinetTensor* u, int kT, int& grid) {
  a.To = u->T / kT; a.H = u->H; a.W = u->W; a.HW = u->H * u->W;
  a.M = (int)((long)u->B * a.To * a.HW);
  a.dW = make_fastdiv((uint32_t)a.W); a.dHW = make_fastdiv((uint32_t)a.HW); a.dTo = make_fastdiv((uint32_t)a.To);
  // a wave walks up to 32 groups (512 voxels: the weight fragments are loaded once per 64 KB of u), fewer while the grid would
  // not give every CU eight workgroups
  const long groups = ((long)a.M + 15) / 16;
  long gpw = groups / (4L * 256 * 8);
  gpw = gpw < 1 ? 1 : (gpw > 32 ? 32 : gpw);
  a.groups_per_wave = (int)gpw;
  grid = (int)((groups + 4 * gpw - 1) / (4 * gpw));
}

}  // namespace

extern "C" int vinet_decoder_tail_ok(int32_t dtype, const VinetTensor* u, int32_t kT, const void* w_mid, const float* b_mid,
                                     const void* w_head, const float* b_head, const VinetTensor* a6, const float* out) {
  return tail_fwd_args("decoder_tail_ok", dtype, u, kT, w_mid, b_mid, w_head, b_head, a6, out) == 0 ? 1 : 0;
}

extern "C" int vinet_decoder_tail_fwd(int32_t dtype, const VinetTensor* u, int32_t kT, const void* w_mid, const float* b_mid,
                                      const void* w_head, const float* b_head, const VinetTensor* a6, float* out, int64_t sb,
                                      int64_t sh, int64_t sw, void* stream) {
  if (tail_fwd_args("decoder_tail_fwd", dtype, u, kT, w_mid, b_mid, w_head, b_head, a6, out)) return -1;
  TailArgs a{};
  int grid;
  tail_shape(a, u, kT, grid);
  a.u = (const char*)u->ptr; a.u_sB = u->sB; a.u_ld = u->ld;
  if (a6) { a.a6 = (char*)a6->ptr; a.a6_sB = a6->sB; a.a6_ld = a6->ld; }
  a.w_mid = (const char*)w_mid; a.b_mid = b_mid; a.w_head = (const char*)w_head; a.b_head = b_head;
  a.out = out; a.o_sb = sb; a.o_sh = sh; a.o_sw = sw;
  hipStream_t s = (hipStream_t)stream;
  if (kT == 2) hipLaunchKernelGGL(decoder_tail_fwd_kernel<2>, dim3(grid), dim3(256), 0, s, a);
  else if (kT == 3) hipLaunchKernelGGL(decoder_tail_fwd_kernel<3>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(decoder_tail_fwd_kernel<4>, dim3(grid), dim3(256), 0, s, a);
  return vn_launch_status("decoder_tail_fwd");
}

extern "C" int vinet_decoder_tail_bwd(int32_t dtype, const float* g, int64_t gsb, int64_t gsh, int64_t gsw, const float* out,
                                      int64_t sb, int64_t sh, int64_t sw, const VinetTensor* a6, int32_t kT, const void* w_mid_t,
                                      const void* w_head, const VinetTensor* dy_head, const VinetTensor* dz6, const VinetTensor* du,
                                      int32_t accumulate, void* stream) {
  const char* what = "decoder_tail_bwd";
  VN_CHECK_ARG(!accumulate, "%s: du is stored, never accumulated (this pass is the only writer of that gradient)", what);
  VN_CHECK_ARG(tail_view_ok(du, 32), "%s: du must be a 32-channel bf16 view on the 16-byte grid", what);
  if (tail_common_args(what, dtype, du, kT, w_mid_t, w_head, a6, true)) return -1;
  VN_CHECK_ARG(g && out && ((uintptr_t)g % 4) == 0 && ((uintptr_t)out % 4) == 0, "%s: null or misaligned map or map gradient", what);
  VN_CHECK_ARG(tail_view_ok(dz6, 32) && same_dims(*dz6, *a6), "%s: dz6 must be a6's extent, 32 channels, on the 16-byte grid", what);
  VN_CHECK_ARG(tail_view_ok(dy_head, 8) && dy_head->B == a6->B && dy_head->T == a6->T && dy_head->H == a6->H && dy_head->W == a6->W,
               "%s: dy_head must be a6's extent, 8 channels (channel 0 real), on the 16-byte grid", what);
  TailArgs a{};
  int grid;
  tail_shape(a, du, kT, grid);
  a.a6 = (char*)a6->ptr; a.a6_sB = a6->sB; a.a6_ld = a6->ld;
  a.w_mid = (const char*)w_mid_t; a.w_head = (const char*)w_head;
  a.out = (float*)out; a.o_sb = sb; a.o_sh = sh; a.o_sw = sw;
  a.g = g; a.g_sb = gsb; a.g_sh = gsh; a.g_sw = gsw;
  a.dy = (char*)dy_head->ptr; a.dy_sB = dy_head->sB; a.dy_ld = dy_head->ld;
  a.dz = (char*)dz6->ptr; a.dz_sB = dz6->sB; a.dz_ld = dz6->ld;
  a.du = (char*)du->ptr; a.du_sB = du->sB; a.du_ld = du->ld;
  hipStream_t s = (hipStream_t)stream;
  if (kT == 2) hipLaunchKernelGGL(decoder_tail_bwd_kernel<2>, dim3(grid), dim3(256), 0, s, a);
  else if (kT == 3) hipLaunchKernelGGL(decoder_tail_bwd_kernel<3>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(decoder_tail_bwd_kernel<4>, dim3(grid), dim3(256), 0, s, a);
  return vn_launch_status("decoder_tail_bwd");
}
