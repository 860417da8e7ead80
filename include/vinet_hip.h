/*
 * vinet_hip.h -- C ABI of libvinet_hip.so: the MI355X (gfx950) kernels behind
 * the ViNet / AViNet saliency hot path.
 *
 * The reference (samyak0210/ViNet) has no FFI seam of its own: its hot path is
 * `nn.Module`s calling aten.  The seam this library fills is therefore "the
 * aten ops that model_utils.py / model.py / loss.py execute", one entry point
 * per kernel family x direction.  Each declaration cites the reference call
 * site(s) (file:line under /root/reference) whose device work it replaces.
 *
 * Conventions
 *  - plain C, POD structs, no torch types.  All pointers are DEVICE pointers
 *    unless named `host_*`.
 *  - the caller owns every buffer (inputs, outputs, workspaces).  The library
 *    allocates nothing, creates no streams and never synchronises: work is
 *    enqueued on the `hipStream_t` passed in (as `void*`), on the device that
 *    is current for the calling thread.
 *  - re-entrant; safe to call from several host threads (one per device /
 *    autograd worker threads).
 *  - return value: 0 = ok; negative = invalid argument (see
 *    vinet_last_error()); positive = hipError_t from the launch.
 *  - activations are CHANNELS-LAST 5-D views `[B][T][H][W][C]` (the torch
 *    `channels_last_3d` memory format of a logical NCDHW tensor), described by
 *    VinetTensor: W-stride `ld` elements (>= C, so a view may be a channel
 *    slice of a wider concat buffer), H-stride `W*ld`, T-stride `H*W*ld`,
 *    batch stride `sB` (so a view may also be a T slice of a longer buffer).
 *  - dtype: VINET_F32 (parity path) or VINET_BF16 (throughput path); all
 *    accumulation, BN statistics and loss arithmetic are fp32/fp64.  Conv and
 *    weight-gradient descriptors (and vinet_pack_weights) also take VINET_F32S:
 *    fp32 tensors, bf16 matrix arithmetic on hi / lo halves of both operands.
 */
#ifndef VINET_HIP_H
#define VINET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VINET_ABI_VERSION 16   /* still 16: vinet_token_encoder_fwd / _bwd / _workspace and vinet_token_split_fwd / _bwd are pure additions; vinet_emd, vinet_emd_hist and vinet_emd_workspace are pure additions as well; vinet_auc_borji, vinet_auc_borji_workspace and vinet_info_gain are pure additions (no existing entry point or struct changed); 16: vinet_auc_shuffled, vinet_auc_shuffled_workspace; 15: vinet_transformer_fwd / _bwd / _workspace; 14: vinet_auc_judd, vinet_auc_judd_workspace; 13 (round 6): tline 5 / 1 also promise weight slices < 64 */

enum { VINET_F32 = 0, VINET_BF16 = 1,
       /* conv / weight-gradient descriptors only: fp32 tensors (as VINET_F32), bf16 matrix arithmetic on a two-term split of both
        * operands (x = hi + lo, 16 significant bits; hi*hi + hi*lo + lo*hi, fp32 accumulate) -- 3/16 of the fp32-MFMA cost, error
        * ~2^-17 per operand.  The fast configuration that still meets north_star's 1e-3 / exact-argmax contract. */
       VINET_F32S = 2 };
enum { VINET_ACT_NONE = 0, VINET_ACT_RELU = 1, VINET_ACT_SIGMOID = 2 };
enum { VINET_CONV_GENERIC = 0, VINET_CONV_STEM = 1 };

typedef struct VinetTensor {
  void* ptr;      /* element [0,0,0,0,0] of the view */
  int32_t B, T, H, W, C;
  int32_t ld;     /* elements between consecutive W positions */
  int64_t sB;     /* elements between consecutive batch items */
} VinetTensor;

/* A per-channel affine (+ReLU) applied to a tensor WHILE IT IS LOADED: the
 * consumer-side form of BatchNorm3d(+ReLU) in training mode, where the
 * producer conv stores its raw output and the statistics only exist after the
 * whole tensor has been written (model_utils.py:132-133,145-146,149-150).
 * scale == NULL means identity. */
typedef struct VinetAffine {
  const float* scale;
  const float* shift;
  int32_t relu;
} VinetAffine;

/* ------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA.
 * Replaces nn.Conv3d forward and its two backward halves wherever the
 * reference calls them: model_utils.py:131,144,148 (BasicConv3d / SepConv3d),
 * model.py:256,261,266,271,275,280,282 (decoder), and, with T as the 1-D axis,
 * nn.Conv2d (k,1) of SoundNet model.py:750-791.
 *
 *   y[b, (to,ho,wo) -> storage pos, n] (+)= act( out_scale[n] * sum_{tap,c}
 *        pre(x[b, to*sT+dt_tap, ho*sH+dh_tap, wo*sW+dw_tap, c]) * w[slice_tap][n][c] + out_shift[n] )
 *
 *  - `taps`: ntaps x int32[4] = (dt, dh, dw, weight slice); padding is folded
 *    into the offsets (dt = kt - padT ...), out-of-range reads are zero.  A
 *    transposed convolution (dgrad of a strided conv) is expressed by the
 *    caller as one launch per stride phase with that phase's tap subset.
 *  - `w`: packed [nslices][N][Kp], Kp = Cin rounded up to 32, same dtype as x
 *    (see vinet_pack_weights).
 *  - output storage position = (to*omT+ooT, ho*omH+ooH, wo*omW+ooW) inside
 *    `y`, so producers write straight into concat buffers / phase-strided
 *    gradients (torch.cat at model_utils.py:187, model.py:290,296,302 is never
 *    materialised as a copy).
 *  - `stats` (optional): per-M-tile partial sums of the pre-activation values,
 *    layout [tilesM][2][N] fp32 (sum, sum of squares), tilesM =
 *    vinet_conv3d_stats_rows(desc); reduced by vinet_bn_finalize.
 *  - mode VINET_CONV_STEM: x has C == 4 (3 + zero pad), taps index kernel
 *    rows only and each K chunk of 32 is 8 consecutive W positions x 4
 *    channels (the 1x7x7 stride-2 stem, model.py:693 / model_utils.py:144).
 * ---------------------------------------------------------------------- */
typedef struct VinetConvDesc {
  int32_t dtype;        /* of x and w */
  int32_t out_dtype;    /* of y */
  int32_t mode;         /* VINET_CONV_GENERIC / VINET_CONV_STEM */
  VinetTensor x;        /* C = Cin (multiple of 16 bytes worth of elements) */
  VinetTensor y;        /* output storage, C = N */
  int32_t oT, oH, oW;   /* iteration space; M = B*oT*oH*oW */
  int32_t sT, sH, sW;
  int32_t omT, omH, omW, ooT, ooH, ooW;
  int32_t ntaps;
  const int32_t* taps;
  const void* w;
  int32_t Kp;
  VinetAffine pre;      /* applied to x on load */
  const float* out_scale;
  const float* out_shift;
  int32_t act;
  int32_t accumulate;   /* y += ... */
  float* stats;
  int32_t n_valid;      /* 0 = y.C; else only channels < n_valid have weights /
                           affine (the rest of a channel-padded y gets act(0)) */
  float* splitk_ws;     /* optional fp32 scratch for split-K (low-M, long-K convs: batch-1 inference): at least
                           vinet_conv3d_splitk_bytes(desc) bytes, contents irrelevant on entry and undefined
                           on return; NULL (or too small) = never split */
  int64_t splitk_ws_bytes;
  int32_t tline;        /* 1 = the caller promises a purely temporal kernel: every tap is (dt, 0, 0, slice) and the
                           dt form the contiguous range [-tpad, -tpad + ntaps - 1] in any order (the tap table is
                           device memory, the library cannot look); lets 64 -> 64 channel layers take the
                           frame-streaming kernel (conv_ts.hip).
                           2 = the taps are (0, kh, 0, slice kh), kh = 0..6: the folded RGB stem (row-streaming strip
                           kernel, conv_hs.hip).
                           3 = not a tap promise but a different problem: the WHOLE data gradient of a strided
                           temporal conv in one launch (instead of one launch per stride phase): x = dy, y = dx,
                           w = the transposed pack, ntaps / sT / tpad = kernel length, stride and padding of the
                           FORWARD conv, oT = y.T; `taps` is ignored.  Only where
                           vinet_conv3d_fuses_dgrad_phases(desc) returns 1.
                           5 = 3 x 3 spatial footprint: every tap is (dt, dh, dw, slice) with |dh| <= 1 and |dw| <= 1, and
                           taps of equal dt are contiguous in the table (ConvPlan.fwd_taps order and every stride phase of
                           its data gradient): lets plain-input layers take the halo-tile kernel (conv_ht.h), which
                           stages the activation patch once per (dt, 64 channels) instead of once per tap.  The weight
                           slice of a tap must be < 64 (six bits of the kernel's packed tap word; the net's largest
                           kernel, 5 x 3 x 3, has 45).  tline 1 (temporal line) carries the same promise for conv_ht's
                           temporal mode.
                           6 = pointwise: ntaps == 1 and the tap is (0, 0, 0, slice 0) (a 1x1x1 / stride-1 conv or its data
                           gradient): lets large problems take the wave-streaming kernel (conv_pw.h), which keeps the
                           weight tile in LDS and feeds the activations to the matrix cores straight from registers.
                           0 = no promise. */
  int32_t tpad;
  /* Optional, data gradients only (ABI 11): y is the gradient g behind a BatchNorm (+ ReLU) whose RAW input is bnb_z -- same
   * extent as y, rows of bnb_ld elements, clips bnb_sB elements apart, dtype of y; bnb_fwd = the forward affine of that
   * BatchNorm (scale, shift, relu: the ReLU gate is scale * z + shift > 0), bnb_mean / bnb_invstd its batch statistics.
   * With bnb_partials != NULL the launch ALSO writes the partial sums of vinet_bn_bwd_reduce(g, z) -- [rows][2][C] fp32,
   * rows = vinet_conv3d_bn_bwd_stats_rows(desc) -- so the caller skips that pass (train.py:193 -> model_utils.py:145: the
   * stem's first BatchNorm, whose gradient comes out of the fused temporal data gradient, tline == 3; ABI 12: every BatchNorm
   * whose output gradient is last written by a data gradient of the shared conv epilogue -- model_utils.py:132,145,149).  The sums
   * are formed on the values the launch STORES (rounded to y's dtype; with accumulate != 0 on old + new, so the caller must make
   * this launch the last writer of y).  Only where the rows query returns > 0.  tline == 3: accumulate must be 0. */
  const void* bnb_z;
  int32_t bnb_ld;
  int64_t bnb_sB;
  VinetAffine bnb_fwd;
  const float* bnb_mean;
  const float* bnb_invstd;
  float* bnb_partials;
} VinetConvDesc;

int vinet_conv3d(const VinetConvDesc* desc, void* stream);
/* Bytes of fp32 scratch with which vinet_conv3d would split this problem's K loop over several workgroups
 * (each split stores its partial sums to its own slab; a finishing pass adds the slabs in a fixed order, so the
 * result is run-to-run deterministic, and applies the epilogue); 0 when it would not split (enough tiles,
 * short K, statistics or accumulate requested). */
int64_t vinet_conv3d_splitk_bytes(const VinetConvDesc* desc);
/* 1 if vinet_conv3d accepts this tline == 3 descriptor (fused stride phases of a temporal data gradient). */
int vinet_conv3d_fuses_dgrad_phases(const VinetConvDesc* desc);
/* Rows of BatchNorm-backward partial sums ([rows][2][C] fp32) that vinet_conv3d writes for this descriptor when bnb_partials is
 * set (bnb_z, bnb_ld, bnb_sB, bnb_fwd, bnb_mean, bnb_invstd filled in; bnb_partials itself is not looked at); 0 = the kernel
 * this problem takes cannot fold the reduce pass in: leave bnb_partials NULL and call vinet_bn_bwd_reduce. */
int vinet_conv3d_bn_bwd_stats_rows(const VinetConvDesc* desc);
/* 1 if the kernel vinet_conv3d picks for this problem applies the pending affine `pre` ONCE per staged activation (the
 * halo-tile kernel transforms its LDS image in place) rather than at every fragment read: callers that would otherwise
 * materialise relu(bn(x)) with vinet_copy_affine first can skip that pass. */
int vinet_conv3d_applies_pre_once(const VinetConvDesc* desc);
/* BM of the tile configuration vinet_conv3d will pick for this problem. */
int vinet_conv3d_tile_m(const VinetConvDesc* desc);
/* Rows of the `stats` table ([rows][2][N]) the launch fills: ceil(M / tile_m) for the row-tiled kernels, the number
 * of spatial tiles for the halo-tile kernel (partial tiles at the image border).  Size `stats` with this. */
int vinet_conv3d_stats_rows(const VinetConvDesc* desc);
/* Name of the kernel instantiation vinet_conv3d will launch for this problem
 * (profilers report kernels by that name). */
int vinet_conv3d_kernel_name(const VinetConvDesc* desc, char* buf, int32_t n);

/* Weight gradient: dw[slice_tap][n][c] (+)= sum_m dy[m][n] * pre(x[m shifted by tap])[c]
 * (the wgrad half of convolution_backward, train.py:216).  `dw` is fp32
 * [nslices][N][Kp] and MUST be zero on entry (split-K partial products are
 * accumulated with fp32 atomics); vinet_unpack_wgrad converts it to the
 * torch [N][Cin][kT][kH][kW] layout. */
typedef struct VinetWgradDesc {
  int32_t dtype;
  int32_t mode;
  VinetTensor x;
  VinetTensor dy;       /* [B][oT][oH][oW][N] */
  int32_t sT, sH, sW;
  int32_t ntaps;
  const int32_t* taps;
  float* dw;
  int32_t Kp;
  VinetAffine pre;
  int32_t tline;        /* 1 = the caller promises a purely temporal kernel: tap kt is (kt - tpad, 0, 0, slice kt),
                           kt = 0..ntaps-1 (the tap table lives in device memory, the library cannot look);
                           lets 64 -> 64 channel layers take the frame-streaming kernel.
                           2 = the taps are (0, kh, 0, slice kh), kh = 0..6: the folded RGB stem (row-streaming strip
                           kernel).
                           4 = the taps are (kt, kh-1, kw-1, slice (kt*3 + kh)*3 + kw), kt < ntaps / 9: a kT x 3 x 3
                           kernel with stride (kT,1,1), padding (0,1,1) (the decoder convs; row-streaming kernel for
                           64 output channels).  0 = no promise. */
  int32_t tpad;
  /* Optional fused BatchNorm(+ReLU) backward.  With bnb_z != NULL, `dy` is the gradient w.r.t. the OUTPUT of the
   * BatchNorm that follows this conv, bnb_z the raw conv output (same B/T/H/W/C as dy), and the kernel forms
   *   dz = scale * (dy * mask - c1 - (z - mean) * invstd * c2)        (vinet_bn_bwd_apply's arithmetic, rounded to
   * the activation dtype) on the fly instead of reading a stored dz: for a conv whose input needs no gradient (the
   * RGB stem) dz has no other consumer, so the apply pass (2 reads + 1 write of the layer's largest tensor) and
   * the wgrad's own read of dz become 2 reads.  Only kernels that say so support it: ask
   * vinet_conv3d_wgrad_fuses_bn_bwd(desc) first; vinet_conv3d_wgrad rejects the descriptor otherwise. */
  const void* bnb_z;
  int32_t bnb_ld;
  int64_t bnb_sB;
  VinetAffine bnb_fwd;           /* forward scale / shift / relu of that BatchNorm */
  const float* bnb_mean;
  const float* bnb_invstd;
  const float* bnb_c1;
  const float* bnb_c2;
  /* Compute units the PERSISTENT weight-gradient kernels (one 512-thread workgroup per CU: the row- and frame-streaming
   * forms) may occupy for this launch: a caller that runs its weight gradients on a second stream beside the data-gradient
   * chain leaves the rest of the chip to that chain.  0 = the whole chip (256).  Per launch and per descriptor, so that
   * concurrent callers (one host thread per device, autograd worker threads) never share mutable state. */
  int32_t max_cus;
} VinetWgradDesc;

int vinet_conv3d_wgrad(const VinetWgradDesc* desc, void* stream);
/* 1 if vinet_conv3d_wgrad would apply desc->bnb_* itself for this problem (fill the bnb_* fields before asking). */
int vinet_conv3d_wgrad_fuses_bn_bwd(const VinetWgradDesc* desc);
int vinet_conv3d_wgrad_kernel_name(const VinetWgradDesc* desc, char* buf, int32_t n);

/* fp32 torch-layout master weights [N][Cin][ntaps] -> packed compute weights.
 *  transpose == 0: out[t][n][c]       (Kp = pad32(Cin))   forward / wgrad layout
 *  transpose == 1: out[t][c][n]       (Kp = pad32(N))     dgrad layout
 *  stem      == 1: out[kh][n][kw*4+c] (Kp = 32; ntaps = 7*7, Cin = 3)
 * dtype VINET_F32S (the packs VINET_F32S descriptors read): the same logical arrays, stored as hi / lo bf16 planes -- every
 * 32-wide K chunk of a row becomes 128 bytes [32 bf16 hi | 32 bf16 lo], hi = bf16(w), lo = bf16(w - hi), K positions permuted so
 * that positions 8q .. 8q+7 hold channels {4q .. 4q+3, 16+4q .. 16+4q+3} (the order in which the kernels' lane groups read fp32
 * activations in 16-byte pieces).  Same byte count as the fp32 pack; callers size the buffer as for VINET_F32.
 * Replaces the implicit weight reads of every nn.Conv3d above. */
int vinet_pack_weights(const float* w, int32_t N, int32_t Cin, int32_t ntaps, int32_t transpose, int32_t stem,
                       int32_t dtype, void* out, void* stream);

/* Multi-tensor vinet_pack_weights: one launch for every weight of the model (they all go stale together
 * after the optimizer step; replaces ~170 launches of model_utils.py conv weights per training step).
 * `table` is DEVICE memory: (njobs + 1) rows of 8 int64
 *   { w (const float*), out (packed, dtype), N, Cin, ntaps, transpose | stem << 1, first output index, ld | col << 32 }
 * the last row carrying only the total in its prefix field; layouts exactly as vinet_pack_weights.  A transposed
 * job with ld != 0 writes its N columns at [col, col + N) of rows `ld` elements apart (padding columns are the
 * caller's to zero): the 1x1x1 convs of an Inception block that share an input are packed side by side along K
 * so that their data gradients are ONE conv (model_utils.py:176-187). */
int vinet_pack_weights_multi(const int64_t* table, int32_t njobs, int64_t total, int32_t dtype, void* stream);
/* packed fp32 dw -> torch layout; grad (+)= dw.  flags: bit 0 = accumulate into grad (else store), bit 1 = hand
 * `dw` back ZEROED (rows [0,N) of every slice, padding columns included), so a caller-owned persistent workspace
 * meets vinet_conv3d_wgrad's "zero on entry" contract at the next step without a fill launch. */
int vinet_unpack_wgrad(float* dw, int32_t N, int32_t Cin, int32_t ntaps, int32_t stem, int32_t flags,
                       float* grad, void* stream);
/* Multi-tensor vinet_unpack_wgrad: the weight gradients of a whole backward pass (train.py:216; 84 Conv3d weights of
 * ViNet-32, model.py / model_utils.py) handed to their `.grad` tensors in one launch.  `table` is DEVICE memory:
 * (njobs + 1) rows of 8 int64 { dw (packed fp32), grad (torch layout fp32), N, Cin, ntaps, stem, first PACKED index, 0 },
 * the last row carrying only the total number of packed elements in its prefix field (a job has nsl * N * Kp of them:
 * nsl = 7 / Kp = 32 for the stem, ntaps / rup(Cin, 32) otherwise).  `flags` as vinet_unpack_wgrad, for every job. */
int vinet_unpack_wgrad_multi(const int64_t* table, int32_t njobs, int64_t total, int32_t flags, void* stream);

/* ------------------------------------------------------------------------
 * Layout / dtype conversion at the module boundary.
 * NCDHW-logical fp32 tensor with arbitrary element strides (train.py:205
 * hands over a permuted view) -> channels-last, channel-padded `dst`
 * (dst.C >= C, pad channels zeroed); and back.
 * ---------------------------------------------------------------------- */
int vinet_import_ncdhw(const float* src, int64_t sb, int64_t sc, int64_t st, int64_t sh, int64_t sw, int32_t C,
                       const VinetTensor* dst, int32_t dst_dtype, void* stream);
/* Same, into a zero-padded buffer: dst voxel (h, w) <- src(h - pad_top, w - pad_left), zeros
 * elsewhere (src is [.., Hs, Ws]).  Used for the RGB stem: with 3 rows / 3 pixels of padding the
 * 1x7x7 stride-2 conv (model_utils.py:144 via model.py:693) reads, for every output and kernel
 * row, 8 pixels x 4 channels = 64 contiguous, 16-byte aligned, always in-bounds bytes, i.e. it is
 * a generic 7-tap conv over the overlapped view [B][T][Hs+6][(Ws+8)/2][C=32], ld = 8. */
int vinet_import_ncdhw_pad(const float* src, int64_t sb, int64_t sc, int64_t st, int64_t sh, int64_t sw, int32_t C,
                           int32_t Hs, int32_t Ws, int32_t pad_top, int32_t pad_left, const VinetTensor* dst,
                           int32_t dst_dtype, void* stream);
/* dst[b,c,t,h,w] (fp32, strides given) = pre(src); accumulate adds. */
int vinet_export_ncdhw(const VinetTensor* src, int32_t src_dtype, VinetAffine pre, float* dst, int64_t sb, int64_t sc,
                       int64_t st, int64_t sh, int64_t sw, int32_t accumulate, void* stream);
/* channels-last -> channels-last copy with optional affine+relu (materialises
 * a pending BN, writes a skip connection into a T-concat buffer, converts
 * dtype).  dst (+)= pre(src). */
int vinet_copy_affine(const VinetTensor* src, int32_t src_dtype, VinetAffine pre, const VinetTensor* dst,
                      int32_t dst_dtype, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------
 * BatchNorm3d / BatchNorm2d (model_utils.py:132,145,149; model.py:752-786).
 * ---------------------------------------------------------------------- */
/* Training: reduce conv-epilogue partials [rows][2][C] -> batch mean / biased
 * var; write mean, invstd, and the consumer-side affine scale = gamma*invstd,
 * shift = beta - mean*scale; update running stats with `momentum` (unbiased
 * variance), as aten native_batch_norm does. */
/* `ld` (0 = C): row stride of the partials when the C channels are a slice of a wider epilogue's columns. */
int vinet_bn_finalize(const float* partials, int32_t rows, int32_t C, int32_t ld, double count, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                      float* mean, float* invstd, float* scale, float* shift, void* stream);
/* Optional pre-reduction of a tall partials table [rows][2][C] into out[out_rows][2][C] (chunks of
 * ceil(rows / out_rows) consecutive rows; (out_rows - 1) * chunk < rows required), coalesced: the finalize kernels
 * walk the rows with one workgroup per channel, which is slow for the 10^5 rows of the 64-channel stem layers. */
int vinet_bn_partials_fold(const float* partials, int32_t rows, int32_t C, float* out, int32_t out_rows, void* stream);
/* Eval: scale = gamma / sqrt(running_var + eps), shift = beta + (conv_bias - running_mean)*scale. */
int vinet_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                  const float* conv_bias /* optional */, float eps, int32_t C, float* scale, float* shift,
                  float* invstd /* optional */, void* stream);
/* Generic per-channel statistics of a tensor (used when the producer is not a
 * conv epilogue): partials [rows][2][C]; returns rows via vinet_stats_rows.
 * Refused (vinet_channel_stats, vinet_bn_bwd_reduce, vinet_channel_sum alike): more than 256 channel groups that do not fill
 * whole passes of 256 -- groups of 8 channels when every view has C, ld and sB in multiples of 8 and a 16-byte aligned pointer
 * (C > 2048 with C % 2048 != 0), groups of 4 otherwise (C > 1024 with C % 1024 != 0).  The network has nothing past 2048. */
int vinet_channel_stats(const VinetTensor* x, int32_t dtype, float* partials, void* stream);
int vinet_stats_rows(const VinetTensor* x);
/* Backward of y = relu?(scale*x_raw + shift) followed by BN-train statistics:
 *  pass 1: partials[rows][2][C] of (sum dz*mask, sum dz*mask*xhat)
 *  pass 2: dx_raw = scale*(dz*mask - c1 - xhat*c2)   (c1 = c2 = 0 in eval mode)
 * native_batch_norm_backward + threshold_backward (train.py:216).
 * vinet_bn_bwd_reduce: fwd.scale and fwd.shift come together or not at all (one without the other is refused); with neither and
 * relu = 1 the gate is x_raw > 0. */
int vinet_bn_bwd_reduce(const VinetTensor* dz, const VinetTensor* x_raw, int32_t dtype, VinetAffine fwd,
                        const float* mean, const float* invstd, float* partials, void* stream);
int vinet_bn_bwd_finalize(const float* partials, int32_t rows, int32_t C, int32_t ld, double count, const float* scale,
                          int32_t train, float* dgamma_acc, float* dbeta_acc, const float* invstd, float* c1, float* c2,
                          void* stream);
int vinet_bn_bwd_apply(const VinetTensor* dz, const VinetTensor* x_raw, int32_t dtype, VinetAffine fwd,
                       const float* mean, const float* invstd, const float* c1, const float* c2,
                       const VinetTensor* dx, void* stream);
/* vinet_bn_bwd_apply on fp32 tensors + vinet_split_bf16 of its result in the same pass: dx as usual and its hi / lo bf16 planes
 * (hi = bf16(v), lo = bf16(v - hi)) -- the operand planes of the VINET_F32S weight gradient (three bf16 launches).  C % 8 == 0. */
int vinet_bn_bwd_apply_split(const VinetTensor* dz, const VinetTensor* x_raw, VinetAffine fwd, const float* mean,
                             const float* invstd, const float* c1, const float* c2, const VinetTensor* dx,
                             const VinetTensor* hi, const VinetTensor* lo, void* stream);
/* dy = dz * act'(z) for z = relu(.) or sigmoid(.) outputs (threshold_backward /
 * sigmoid_backward of the decoder, model.py:257-283).  z may be fp32. */
int vinet_act_bwd(const VinetTensor* dz, int32_t dz_dtype, const VinetTensor* z, int32_t z_dtype, int32_t act,
                  const VinetTensor* dy, int32_t dy_dtype, void* stream);
/* per-channel sum over all voxels (conv bias gradients):
 * out[j] (+)= sum over voxels and over channels c with c % Cout == j.
 * workspace: fp32 [vinet_stats_rows(x)][2][x.C]. */
int vinet_channel_sum(const VinetTensor* x, int32_t dtype, float* workspace, int32_t Cout, float* out,
                      int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------
 * MaxPool3d (model.py:696,700,705,713,714, model_utils.py:178, model.py:229;
 * MaxPool2d (k,1) of SoundNet model.py:753,759,774 with T as the pooled axis).
 * -inf padding, first maximum in (t,h,w) scan order wins ties.  `argmax`
 * (optional, uint8 [B][oT][oH][oW][C] dense) holds the window-relative tap
 * index for the backward gather.  `pre` has a scale AND a shift, or neither:
 * a scale with a NULL shift is rejected (both entry points and the name query
 * return -1 before any route or launch).
 * ---------------------------------------------------------------------- */
typedef struct VinetPoolDesc {
  int32_t dtype;
  int32_t kT, kH, kW, sT, sH, sW, pT, pH, pW;
} VinetPoolDesc;
int vinet_maxpool3d(const VinetPoolDesc* d, const VinetTensor* x, VinetAffine pre, const VinetTensor* y,
                    uint8_t* argmax, void* stream);
int vinet_maxpool3d_bwd(const VinetPoolDesc* d, const VinetTensor* dy, const uint8_t* argmax, const VinetTensor* dx,
                        int32_t accumulate, void* stream);
/* Name of the kernel the call with these very arguments will launch, with its dtype: "maxpool_fwd8_kernel<bf16>",
 * "maxpool_k3s1_pk_kernel" (pure host code: the pointers are tested for null and alignment only). */
int vinet_maxpool3d_kernel_name(const VinetPoolDesc* d, const VinetTensor* x, VinetAffine pre, const VinetTensor* y,
                                const uint8_t* argmax, char* buf, int32_t n);
int vinet_maxpool3d_bwd_kernel_name(const VinetPoolDesc* d, const VinetTensor* dy, const uint8_t* argmax,
                                    const VinetTensor* dx, char* buf, int32_t n);
/* vinet_maxpool3d that ALSO stores pre(x), rounded to bf16, to the view `keep`: x's B/T/H/W/C with any ld / sB / base pointer (a T
 * slice of a longer buffer, a channel slice).  y and argmax are bit-identical to vinet_maxpool3d's; `keep` holds what
 * vinet_copy_affine(x, pre) would have written, up to the sign of a zero behind a ReLU (integer max after rounding, not fmaxf before
 * it).  Each lane stores the window taps with index in [p, p + s) of every dimension, so no element is loaded or transformed twice.
 * Served: bf16, the route maxpool_fwd8_pk_kernel (the default for every bf16 window but 3x3x3/s1/p1 on 8-channel views), `keep` in
 * whole groups of 8 channels on 16-byte addresses, and in every dimension k >= p + s and out * s >= in, so that the owned taps tile
 * the input: 1x3x3/s(1,2,2)/p(0,1,1), 3x3x3/s2/p1, (2,1,1)/s(2,1,1) at even T, (1,2,2)/s(1,2,2) at even H and W.  Not served: fp32,
 * the LDS / T-walking 3x3x3/s1 kernels, the 4-channel kernels, lib option pool_pk = 0, a stride that leaves input uncovered (odd T
 * under (2,1,1)/s2).  vinet_maxpool3d_keep_ok: 1 if this very call is served, else 0 with the reason in vinet_last_error; the entry
 * point itself returns -1 on such a call and launches nothing. */
int vinet_maxpool3d_keep_ok(const VinetPoolDesc* d, const VinetTensor* x, VinetAffine pre, const VinetTensor* y,
                            const uint8_t* argmax, const VinetTensor* keep);
int vinet_maxpool3d_keep(const VinetPoolDesc* d, const VinetTensor* x, VinetAffine pre, const VinetTensor* y,
                         uint8_t* argmax, const VinetTensor* keep, void* stream);
/* BatchNorm backward behind the 1x3x3 / s(1,2,2) / p(0,1,1) pool, the pool's backward folded in: the gradient dz behind
 * relu(bn(z)) is never stored.  Both passes form it in registers exactly as vinet_maxpool3d_bwd(pool, dp, argmax, gacc, accumulate)
 * would have stored it (bf16, + the old contents of `gacc` when `accumulate`) and continue as vinet_bn_bwd_reduce /
 * vinet_bn_bwd_apply: the partials have vinet_stats_rows(z) rows of [2][C] for vinet_bn_bwd_finalize (the same terms as the unfused
 * reduce, partitioned differently), dx is bit-identical to the three-call chain.  dx may be gacc (in place); gacc may be NULL
 * without `accumulate`.  vinet_bn_bwd_pool_ok: 1 if the two entry points take this problem -- bf16, C in whole groups of 8 on
 * 16-byte views, that pool geometry, dp the pooled shape of z, dx the shape of z -- else 0 with the reason in vinet_last_error;
 * the entry points themselves return -1 on such a problem and launch nothing. */
int vinet_bn_bwd_pool_ok(const VinetPoolDesc* pool, const VinetTensor* z, const VinetTensor* dp, const VinetTensor* dx, int32_t dtype);
int vinet_bn_bwd_reduce_pool(const VinetPoolDesc* pool, const VinetTensor* dp, const uint8_t* argmax, const VinetTensor* gacc,
                             int32_t accumulate, const VinetTensor* z, int32_t dtype, VinetAffine fwd, const float* mean,
                             const float* invstd, float* partials, void* stream);
int vinet_bn_bwd_apply_pool(const VinetPoolDesc* pool, const VinetTensor* dp, const uint8_t* argmax, const VinetTensor* gacc,
                            int32_t accumulate, const VinetTensor* z, int32_t dtype, VinetAffine fwd, const float* mean,
                            const float* invstd, const float* c1, const float* c2, const VinetTensor* dx, void* stream);

/* nn.Upsample(scale_factor=(1,2,2), mode='trilinear', align_corners=False)
 * (model.py:254,258,263,268,273,278) and its backward. */
int vinet_upsample2x(const VinetTensor* x, const VinetTensor* y, int32_t dtype, void* stream);
int vinet_upsample2x_bwd(const VinetTensor* dy, const VinetTensor* dx, int32_t dtype, int32_t accumulate, void* stream);
/* The same with the backward of the ReLU in FRONT of the upsample folded in (the decoder's conv -> ReLU -> upsample,
 * model.py:256-258): dx = [xf > 0] * upsample2x^T(dy), xf = the ReLU's output (the upsample's input, dx's extent).  Stores. */
int vinet_upsample2x_bwd_relu(const VinetTensor* dy, const VinetTensor* dx, const VinetTensor* xf, int32_t dtype, void* stream);

/* ----------------------------------------------------------------------
 * The decoder tail behind the last upsample (csrc/decoder_tail.hip), one pass forward and one backward:
 *   u [B, kT, H, W, 32] -> conv 32->32 (kT,1,1)/s(kT,1,1) (+ b_mid) -> ReLU -> a6 [B, 1, H, W, 32]
 *                       -> conv 32->1 + b_head -> sigmoid -> out [B, H, W] fp32 (element strides sb, sh, sw)
 * vinet_decoder_tail_fwd: w_mid / w_head are the FORWARD packs of the two convs exactly as vinet_conv3d gets them (bf16,
 * vinet_pack_weights: [kT][32][32] and [1][32]); b_mid may be NULL, b_head not; a6 may be NULL (inference: not stored).  out and
 * a6 hold the bits of vinet_conv3d (ReLU) + vinet_conv3d (8-channel-padded fp32 head, sigmoid) + vinet_export_ncdhw.
 * vinet_decoder_tail_bwd: g = the gradient of `out` (fp32, own strides), w_mid_t the TRANSPOSED pack of the mid conv, w_head the
 * forward pack of the head.  Writes dy_head [B, 1, H, W, 8] bf16 = bf16(g s (1 - s)) in channel 0 and zeros in channels 1..7,
 * dz6 (a6's extent) = [a6 > 0] bf16(w_head dy_head), du (u's extent) = dz6 . W_mid per tap -- the bits of vinet_import_ncdhw +
 * vinet_act_bwd (sigmoid) + the head's data gradient + vinet_act_bwd (ReLU) + the kT per-tap data gradients.  du is STORED:
 * `accumulate` must be 0.  The weight and bias gradients of both convs stay with vinet_conv3d_wgrad / vinet_channel_sum over
 * (u, dz6) and (a6, dy_head).
 * Served: bf16, kT in {2, 3, 4}, u.T == kT (one output frame, as in every decoder), every view in whole groups of 8 channels on 16-byte addresses, packs on
 * 16-byte addresses, out / g on 4-byte addresses.  vinet_decoder_tail_ok: 1 if the forward call with these arguments is served, else 0
 * with the reason in vinet_last_error; it never launches.  The entry points return -1 on what is not served and launch nothing.
 * ---------------------------------------------------------------------- */
int vinet_decoder_tail_ok(int32_t dtype, const VinetTensor* u, int32_t kT, const void* w_mid, const float* b_mid, const void* w_head,
                          const float* b_head, const VinetTensor* a6, const float* out);
int vinet_decoder_tail_fwd(int32_t dtype, const VinetTensor* u, int32_t kT, const void* w_mid, const float* b_mid, const void* w_head,
                           const float* b_head, const VinetTensor* a6, float* out, int64_t sb, int64_t sh, int64_t sw, void* stream);
int vinet_decoder_tail_bwd(int32_t dtype, const float* g, int64_t gsb, int64_t gsh, int64_t gsw, const float* out, int64_t sb,
                           int64_t sh, int64_t sw, const VinetTensor* a6, int32_t kT, const void* w_mid_t, const void* w_head,
                           const VinetTensor* dy_head, const VinetTensor* dz6, const VinetTensor* du, int32_t accumulate, void* stream);

/* SoundNet's first conv (model.py:751: Conv2d(1, 16, (64,1), stride (2,1), padding (32,0))) as a pointwise conv over the
 * unfolded waveform: y[b, m, 0, 0, c] = x[b, stride*m - pad + c, 0, 0, channel 0], zero outside; x = [B][L][1][1][C>=1],
 * y = [B][(L + 2 pad - k)/stride + 1][1][1][k], k = y.C (a multiple of 8).  The conv's weight [N][1][k][1] is, flat, the
 * pointwise weight [N][k]. */
int vinet_unfold1d(const VinetTensor* x, const VinetTensor* y, int32_t dtype, int32_t stride, int32_t pad, void* stream);

/* ------------------------------------------------------------------------
 * Losses (loss.py:13-99): per-sample reductions in fp64, maps fp32 (or fp64
 * ground truth).  `which`: 0 kldiv, 1 cc, 2 similarity, 3 nss (loss.py:101-120, the
 * validation metric; forward only, vinet_loss_bwd rejects it).
 *  fwd: per_sample[b] and the batch mean in *loss (fp32, device);
 *       `saved` (fp64 [B][8]) keeps the per-sample reductions for backward.
 *  bwd: ds[b,i] (+)= gscale * dloss/ds.
 * ---------------------------------------------------------------------- */
int vinet_loss_fwd(int32_t which, const float* s, const void* gt, int32_t gt_is_f64, int32_t B, int32_t n,
                   double* saved, float* loss, void* stream);
int vinet_loss_bwd(int32_t which, const float* s, const void* gt, int32_t gt_is_f64, int32_t B, int32_t n,
                   const double* saved, const float* gscale, float coeff, int32_t accumulate, float* ds, void* stream);

/* ------------------------------------------------------------------------
 * AUC-Judd (loss.py:122-213), the fifth validation metric; forward only.  One workgroup per map: `s` [B][n] fp32 or
 * fp64 saliency maps (fp64 is what a map is once jitter noise was added, loss.py:158-160), `fix` [B][n] fp32 or fp64
 * fixation maps (a fixation is `fix > 0`).  Per map: S <- (S - min) / (max - min) in the dtype of `s`; thresholds
 * t_0 >= ... >= t_{N-1} = the normalised values at the N fixations; above_i = #{ p : S_p >= t_i };
 * score = trapz(tp, x = fp), tp = [0, 1/N, ..., 1, 1], fp = [0, ..., (above_i - i - fp_offset) / (n - N), ..., 1], fp64.
 * `fp_offset` 0 reproduces loss.py:189 (0-based i), 1 the MATLAB original it was ported from (AUC_Judd.m:72 subtracts
 * the 1-based index).  score[b] is NaN when map b has no fixation, is constant or holds a NaN (loss.py:143-146,
 * 166-169); n == N divides by zero as numpy does.  nfix[b] = N.  `above` (optional, [B][n] int32) receives the N
 * counts of each map.  Counts are exact integers and the sum has a fixed order: results are bit-reproducible and a
 * map's score does not depend on its neighbours in the batch.
 * Up to 4096 fixations a map is sorted and counted in LDS, beyond that (or with option "auc_ws") in `workspace`, which
 * must hold vinet_auc_judd_workspace(B, n) bytes (8-byte aligned) in either case.  jitter=True is the caller adding
 * noise to `s`; normalize=True and toPlot=True have no counterpart (the first raises TypeError in the reference).
 * auc_shuff (loss.py:215-284) raises TypeError on every input and has no counterpart either.
 * ---------------------------------------------------------------------- */
size_t vinet_auc_judd_workspace(int32_t B, int32_t n);
int vinet_auc_judd(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, int32_t B, int32_t n,
                   int32_t fp_offset, void* workspace, size_t workspace_bytes, double* score, int32_t* nfix,
                   int32_t* above, void* stream);

/* ------------------------------------------------------------------------
 * Shuffled AUC (s-AUC) as the reference's evaluation defines it: code_for_Metrics/AUC_shuffled.m with the other map of
 * createShuffmap1.m and the removal of the frame's own fixations of eval_diem.m:65.  Forward only.  (The Python auc_shuff,
 * loss.py:215-284, raises on every input and stays without a counterpart.)
 *   `s` [B][n] fp32 or fp64 saliency maps, `fix` [B][n] fp32 or fp64 fixation maps (a fixation is `fix > 0`), `other`:
 *   other-fixation maps of `other_kind` 0 uint8 / 1 fp32 / 2 fp64, map b at element b * other_stride (0: one map for the
 *   whole batch, else >= n).
 * Per map: S <- (S - min) / (max - min) in the dtype of `s`; N = #{fix > 0}; other set = { p : other_p > 0 and not
 * fix_p > 0 }, M its size, K = min(N, M); thresholds t_k = k * step in fp64 for k = 0, 1, ... while t_k <= 1 (at most 2048
 * of them: step >= 1/2047).  For each of `nsplits` splits: curfix = S at K distinct locations of the other set,
 * tp_k = #{S at fixations >= t_k} / N, fp_k = #{curfix >= t_k} / K, the points (0,0), (fp_k, tp_k) by descending k, (1,1)
 * and their trapezoid area in fp64; score[b] = the mean over the splits.  (AUC_shuffled.m stops the sweep at the largest value
 * present; the thresholds above it add the point (0,0) again, zero area.)  score[b] is NaN when map b has no fixation, is
 * constant, holds a NaN or has an empty other set.  nfix[b] = N, nother[b] = M.
 * Where the K locations come from:
 *   `samples` != NULL: int32 [B][nsplits][kmax], each row K pixel indices followed by -1; the kernel uses them as they are
 *     (a row that does not hold exactly K indices in [0, n) gives that map NaN);
 *   `samples` == NULL: the device draw.  Location p of split j of a map with frame id f has the 32-bit key
 *     mix32(mix32(p ^ k0) + k1) with (k0, k1) a function of (seed, f, j) alone; the K locations of the other set with the
 *     smallest keys are taken (a radix select; the key is a bijection of p, so there are no ties).  frame_ids: int64 [B] or
 *     NULL for 0 .. B-1.  A map's score depends on (its data, seed, its frame id) and not on the batch around it.
 *   `samples_out` (optional, int32 [B][nsplits][kmax]) receives the locations used, in no particular order, padded with -1;
 *     at most kmax per row are written.
 * Counts are exact integers, every fp64 sum has a fixed order: results are bit-reproducible.  `workspace` must hold
 * vinet_auc_shuffled_workspace(B, n, nsplits, step) bytes, 8-byte aligned (0 = invalid arguments): the per-split areas, each
 * map's counts and the list of its other set.  A workgroup stages that list in LDS up to 8192 locations and reads it from the
 * workspace beyond that (or with option "sauc_ws").
 * ---------------------------------------------------------------------- */
size_t vinet_auc_shuffled_workspace(int32_t B, int32_t n, int32_t nsplits, double step);
int vinet_auc_shuffled(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, const void* other,
                       int32_t other_kind, int64_t other_stride, int32_t B, int32_t n, int32_t nsplits, double step,
                       int64_t seed, const int64_t* frame_ids, const int32_t* samples, int32_t kmax, void* workspace,
                       size_t workspace_bytes, double* score, int32_t* nfix, int32_t* nother, int32_t* samples_out,
                       void* stream);

/* ------------------------------------------------------------------------
 * AUC-Borji (code_for_Metrics/AUC_Borji.m).  Forward only.  `s`, `fix`, the normalisation, the thresholds t_k = k * step, the
 * `>=` comparisons and the trapezoid sum are those of vinet_auc_shuffled; what differs is the set of negative locations: for
 * each of `nsplits` splits N = #{fix > 0} locations drawn from ALL n pixels, uniformly and with replacement (AUC_Borji.m:58,
 * MATLAB's randi: a fixation pixel may be drawn, a pixel may repeat), and tp and fp are both divided by N.  score[b] = the mean
 * of the splits' areas in split order; NaN when map b has at most ONE fixation (AUC_Borji.m:31), is constant or holds a NaN.
 * nfix[b] = N.
 *   `samples` != NULL: int32 [B][nsplits][kmax], each row N pixel indices followed by -1, used as they are (a row that does
 *     not hold exactly N indices in [0, n) gives that map NaN);
 *   `samples` == NULL: the device draw.  Sample j of split q of a map with frame id f is pixel ((uint64)h * n) >> 32 with
 *     h = mix32(mix32(j ^ k0) + k1); (k0, k1) are the shuffled AUC's function of (seed', f, q) with
 *     seed' = seed ^ 0x426f726a69415543, so that the two metrics do not share a stream under one seed.  frame_ids: int64 [B]
 *     or NULL for 0 .. B-1.  A map's score depends on (its data, seed, its frame id) and not on the batch around it.
 *   `samples_out` (optional, int32 [B][nsplits][kmax]) receives sample j at position j, padded with -1; at most kmax per row.
 * Counts are exact integers, every fp64 sum has a fixed order: results are bit-reproducible.  `workspace` must hold
 * vinet_auc_borji_workspace(B, n, nsplits, step) bytes, 8-byte aligned (0 = invalid arguments).
 * ---------------------------------------------------------------------- */
size_t vinet_auc_borji_workspace(int32_t B, int32_t n, int32_t nsplits, double step);
int vinet_auc_borji(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, int32_t B, int32_t n, int32_t nsplits,
                    double step, int64_t seed, const int64_t* frame_ids, const int32_t* samples, int32_t kmax, void* workspace,
                    size_t workspace_bytes, double* score, int32_t* nfix, int32_t* samples_out, void* stream);

/* ------------------------------------------------------------------------
 * Information gain (code_for_Metrics/InfoGain.m, IG.m).  Forward only.  `s` [B][n] and `fix` [B][n] fp32 or fp64; `baseline`
 * fp32 or fp64, map b at element b * baseline_stride (0: one map for the whole batch, else >= n), or NULL (IG.m:28-31).
 * All arithmetic in fp64 on the input values: v = (s - min) / (max - min), p = v / sum(v), the same for the baseline (pb);
 * score[b] = mean over { fix > 0 } of log2(eps + p) - log2(eps + pb), eps = 2^-52; without a baseline the second term is
 * absent.  NaN when map b has no fixation, the map or its baseline is constant, or either holds a NaN.  nfix[b] = N.
 * One workgroup per map, sums in a fixed order: bit-reproducible, independent of the batch.  No workspace.
 * ---------------------------------------------------------------------- */
int vinet_info_gain(const void* s, int32_t s_is_f64, const void* fix, int32_t fix_is_f64, const void* baseline,
                    int32_t baseline_is_f64, int64_t baseline_stride, int32_t B, int32_t n, double* score, int32_t* nfix,
                    void* stream);

/* ------------------------------------------------------------------------
 * Earth mover's distance (code_for_Metrics/EMD.m with FastEMD's emd_hat_gd_metric, extra mass penalty 0).  Forward only.
 * vinet_emd_hist scores ready histograms: P, Q fp64 [B][R*C], the bins of an R x C grid in row-major order, D the Euclidean
 * distance of the bin centres.  As the reference's double wrapper does: m = min(P, Q) per bin is pre-flowed (p = P - m,
 * q = Q - m, negative bins included), ip = floor(p f + 0.5), iq = floor(q f + 0.5), iC = floor(D cf + 0.5) with
 * f = 1e6 / max(sum P, sum Q) (running sums in bin order) and cf = 1e6 / max D; the side with the larger integer sum supplies;
 * K = the minimum of sum flow * iC that ships every unit of the lighter side, the surplus dropped free; score[b] = K / f / cf.
 * cost[b] = K (optional, int64; -1 with a non-zero status) and status[b] (optional, int32): 0, or 1 the augmentation guard
 * was reached, 2 / 3 an internal inconsistency, 4 more than 2^31 - 1 units of mass -- each with a NaN score.  The score is
 * also NaN, with status 0 and cost 0, when max(sum P, sum Q) is not positive and finite (a NaN bin included) or the grid has one bin.
 * vinet_emd starts from the maps: `gt` [B][Hg][Wg] and `s` [B][Hs][Ws], fp32 or fp64, each resized to R x C by the two weight
 * matrices given for it -- fp64, dense, [R][Hg] and [C][Wg] for gt, [R][Hs] and [C][Ws] for s; MATLAB's imresize weights are
 * what vinet_amd.utils.matlab_resize_weights builds -- out[r][c] = sum_w wc[c][w] sum_h wr[r][h] x[h][w], then divided by its
 * sum; P comes from gt, Q from s.  R = ceil(Hg / downsize), C = ceil(Wg / downsize) is checked.  hist_out (optional, fp64
 * [B][2][R*C]) receives P and Q.  A resized map whose sum is zero or that holds a NaN gives NaN.
 * The solver is exact (successive shortest paths on the integers; sums in a fixed order): a map's score and cost are
 * bit-identical alone and in any batch.  At most 512 bins (EMD_MAX_BINS: 12 x 20 = 240 for a 360 x 640 map at downsize 32,
 * 17 x 30 = 510 for 1080 x 1920 at 64): the flow matrix takes up to (bins / 2)^2 int32 of workspace per map, and the guard on the
 * solver's loops, (16 n + 16)(n + 1) Dijkstra rounds for n <= bins nodes, stays at seconds.  More bins, downsize < 1, R * C < 1
 * are refused before any launch.  `workspace` must hold vinet_emd_workspace(B, R, C) bytes, 8-byte aligned (0 = invalid arguments).
 * ---------------------------------------------------------------------- */
size_t vinet_emd_workspace(int32_t B, int32_t R, int32_t C);
int vinet_emd(const void* s, int32_t s_is_f64, int32_t Hs, int32_t Ws, const void* gt, int32_t gt_is_f64, int32_t Hg, int32_t Wg,
              int32_t B, int32_t downsize, int32_t R, int32_t C, const double* w_gt_r, const double* w_gt_c, const double* w_s_r,
              const double* w_s_c, void* workspace, size_t workspace_bytes, double* score, int64_t* cost, int32_t* status,
              double* hist_out, void* stream);
int vinet_emd_hist(const double* P, const double* Q, int32_t B, int32_t R, int32_t C, void* workspace, size_t workspace_bytes,
                   double* score, int64_t* cost, int32_t* status, void* stream);

/* torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8) over one flat fp32 buffer
 * (train.py:188,217). bias corrections are passed by the host. */
int vinet_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float bias_c1, float bias_c2, float grad_scale, void* stream);

/* nn.Bilinear(42, 3, 336) fusion (model.py:230,236):
 *  out[b, o, c] = sum_ij x1[b, i, c] * w[o][i][j] * x2[b, j, c] + bias[o]
 * with x1 = [B][I][C], x2 = [B][J][C], out = [B][O][C] channels-last. */
int vinet_bilinear_fwd(const void* x1, const void* x2, int32_t dtype, const float* w, const float* bias, int32_t B,
                       int32_t C, int32_t I, int32_t J, int32_t O, void* out, void* stream);
int vinet_bilinear_bwd(const void* x1, const void* x2, const void* dout, int32_t dtype, const float* w, int32_t B,
                       int32_t C, int32_t I, int32_t J, int32_t O, void* dx1, void* dx2, float* dw, float* dbias,
                       void* stream);

/* ------------------------------------------------------------------------
 * Transformer fusion of the audio-visual model (model.py:8-69, 211-221, 239-247): PositionalEncoding + a stack of
 * nn.TransformerEncoderLayer(E, H, F) -- post-norm, ReLU, LayerNorm eps, dropout p at the attention weights, after the
 * attention projection, between the two linears and after the second -- over S = 32 tokens (the CHANNELS of the
 * channels-last activation) of E features (its T*H*W positions):  tokens[b][c][f] = x[b][f][c] + pe[c][f].
 *
 * x / y (forward) and dy / dx (backward) are channels-last tensors [B][T][H][W][C = S] with T*H*W = E in `dtype`
 * (VINET_F32S is taken as VINET_F32); everything in between is fp32: exact fp32 products on the fp32-input MFMA, fp32
 * accumulation, fp32 softmax rows and LayerNorm statistics.
 * `params` / `grads`: HOST arrays of L * 12 device pointers, per layer in_proj_weight [3E][E], in_proj_bias,
 * out_proj.weight [E][E], out_proj.bias, linear1.weight [F][E], linear1.bias, linear2.weight [E][F], linear2.bias,
 * norm1.weight, norm1.bias, norm2.weight, norm2.bias.  Backward ADDS each parameter's gradient into grads[i] (null: skipped),
 * summing over clips in a fixed order: two runs agree bit for bit.
 * `ws`: vinet_transformer_workspace(desc) bytes, 16-byte aligned; with train = 1 forward leaves the layers' saved state
 * there (inputs of every GEMM, softmax rows, LayerNorm statistics) and backward must get the same buffer and descriptor.
 * Dropout (p > 0, with or without train = 1; pass p = 0 for eval mode): keep masks are a counter-based hash of (seed, *step, layer, site, element), recomputed by
 * backward.  Forward reads the device counter `step`, keeps the value it drew in the workspace and increments the counter,
 * so a captured and replayed step draws new masks.  `masks` (optional, forward): receives the keep masks as bytes, per layer
 * [B][H][S][S] | [B S][E] | [B S][F] | [B S][E].
 * Limits: S = 32, E % 16 == 0, E <= 384, F % 16 == 0, E / H <= 96.
 * ---------------------------------------------------------------------- */
typedef struct VinetTransformerDesc {
  int32_t dtype;
  int32_t B, S, E, H, F, L;
  int32_t train;
  float p, eps;
  uint64_t seed;
  int64_t* step;
  const float* pe;               /* [S][E] */
  const void* const* params;
  void* const* grads;
  void* ws;
  int64_t ws_bytes;
  uint8_t* masks;
} VinetTransformerDesc;
int64_t vinet_transformer_workspace(const VinetTransformerDesc* desc);
int vinet_transformer_fwd(const VinetTransformerDesc* desc, const VinetTensor* x, const VinetTensor* y, void* stream);
int vinet_transformer_bwd(const VinetTransformerDesc* desc, const VinetTensor* dy, const VinetTensor* dx, void* stream);

/* ------------------------------------------------------------------------
 * Token-wise fusion (model.py:116-189, VideoAudioSaliencyFusionModel): the same PositionalEncoding + encoder stack, with the
 * ROWS of the channels-last activation as tokens and its channels as features:  tokens[b][s][e] = x[b][position s][channel e]
 * + pe[s][e].  x / y / dy / dx are views [B][T][H][W][C = E] with T*H*W = S, any ld >= C and any sB (position s of clip b at
 * b sB + s ld); y may be a channel sub-view of a wider tensor, bytes outside the views are not touched.
 * Arithmetic, parameter order, gradient accumulation, null gradients (grads[i] == NULL / dx == NULL are skipped), dropout
 * (sites, stream 4 layer + site, device step counter) and the mask export layout are those of vinet_transformer_* above.
 * Softmax rows are saved by forward; the workspace holds every clip's matrices on S rounded up to 16 rows.
 * Limits: 1 <= S <= 1024, E % 16 == 0, E <= 512, F % 16 == 0, E % H == 0, E / H <= 128, (E / H) % 4 == 0, 0 <= p < 1.
 * ---------------------------------------------------------------------- */
typedef struct VinetTokenEncoderDesc {
  int32_t dtype;
  int32_t B, S, E, H, F, L;
  int32_t train;
  float p, eps;
  uint64_t seed;
  int64_t* step;
  const float* pe;               /* [S][E] */
  const void* const* params;
  void* const* grads;
  void* ws;
  int64_t ws_bytes;
  uint8_t* masks;
} VinetTokenEncoderDesc;
int64_t vinet_token_encoder_workspace(const VinetTokenEncoderDesc* desc);
int vinet_token_encoder_fwd(const VinetTokenEncoderDesc* desc, const VinetTensor* x, const VinetTensor* y, void* stream);
int vinet_token_encoder_bwd(const VinetTokenEncoderDesc* desc, const VinetTensor* dy, const VinetTensor* dx, void* stream);
/* Arithmetic of the encoder's LINEAR products (the six linears of a layer with their data and weight gradients; attention,
 * softmax, LayerNorm, epilogues, workspace and saved activations stay fp32 in every mode), chosen per call whatever `dtype` is:
 *   VINET_TK_MMA_F32     exact fp32 products on the fp32-input MFMA: what the three entry points above run.
 *   VINET_TK_MMA_BF16X3  fp32 matrices, bf16 matrix arithmetic on the two-term split of both operands that VINET_F32S names
 *                        (a = hi + lo, hi = bf16(a) to nearest even, lo = bf16(a - hi), 16 significant bits;
 *                        hi*hi + hi*lo + lo*hi, fp32 accumulate) -- 3/16 of the fp32-MFMA cost, error ~2^-17 per operand.
 *   VINET_TK_MMA_BF16    hi*hi alone, fp32 accumulate: 1/16 of the fp32-MFMA cost, error ~2^-9 per operand.
 * The operands are rounded while they are staged; nothing rounded is stored.  The dropout keep masks of a step do not depend on
 * the mode.  The workspace has one size for all modes.  Backward must be given the mode of its forward.  An unknown mode: -1. */
enum { VINET_TK_MMA_F32 = 0, VINET_TK_MMA_BF16X3 = 1, VINET_TK_MMA_BF16 = 2 };
int64_t vinet_token_encoder_workspace_mma(const VinetTokenEncoderDesc* desc, int32_t mma);
int vinet_token_encoder_fwd_mma(const VinetTokenEncoderDesc* desc, int32_t mma, const VinetTensor* x, const VinetTensor* y, void* stream);
int vinet_token_encoder_bwd_mma(const VinetTokenEncoderDesc* desc, int32_t mma, const VinetTensor* dy, const VinetTensor* dx, void* stream);
/* Arithmetic of ATTENTION, a second selector beside `mma` with the same VINET_TK_MMA_* values; it applies to all seven products:
 *   scores = (q qscale) k^T   AO = (p m) v   dP = dAO v^T   dQ = dS k   dV = (P m)^T dAO   dK = dS^T q
 * (p m: the softmax value times the keep mask and 1 / (1 - p); q qscale is scaled in fp32, then split; dK takes the unscaled q).
 *   F32 = the kernels the entry points above run (fp32-input MFMA);  BF16 = sum hi hi;  BF16X3 = sum (hi hi + hi lo + lo hi),
 * each operand split after it has been formed in fp32, fp32 accumulation inside v_mfma_f32_16x16x32_bf16.  The row maximum, expf,
 * the row sum and the normalisation, the keep-mask draw (a step's masks do not depend on the mode), dS = P (dP m - dot) qscale,
 * the row dots and the values saved in P stay fp32.  Same workspace, same size (any attn), same limits, no atomics, bit-identical
 * runs.  The _mma entry points call these with attn = F32; backward must be given the attn of its forward.  Unknown attn: -1. */
int64_t vinet_token_encoder_workspace_attn(const VinetTokenEncoderDesc* desc, int32_t mma, int32_t attn);
int vinet_token_encoder_fwd_attn(const VinetTokenEncoderDesc* desc, int32_t mma, int32_t attn, const VinetTensor* x, const VinetTensor* y, void* stream);
int vinet_token_encoder_bwd_attn(const VinetTokenEncoderDesc* desc, int32_t mma, int32_t attn, const VinetTensor* dy, const VinetTensor* dx, void* stream);
/* one attention stage without dropout in the arithmetic `attn`, on caller-owned fp32 matrices in the workspace's row layout (every
 * clip owns Sp = S rounded up to 16 rows): qkv [B Sp][3E] (q | k | v, head h at columns h E / H), P [B][H][S][S], ao / dao [B Sp][E],
 * dot [B Sp][H], dqkv [B Sp][3E].  Forward writes P and ao (zeros in ao's padding rows).  Backward READS P and ao (they need not come
 * from a forward), writes dot = rowsum(dao ao) per head and dqkv (zeros in its padding rows).  Limits: those of the descriptor
 * (S, E, E / H); qkv, ao, dao, dqkv 16-byte aligned.  Anything else is refused (-1, vinet_last_error) before a device is touched. */
int vinet_token_attn_fwd(int32_t attn, const float* qkv, int32_t B, int32_t S, int32_t E, int32_t H, float* P, float* ao, void* stream);
int vinet_token_attn_bwd(int32_t attn, const float* qkv, const float* P, const float* dao, const float* ao, int32_t B, int32_t S, int32_t E,
                         int32_t H, float* dot, float* dqkv, void* stream);
/* one linear product of the encoder, any mode (mma = F32 runs tf_gemm): form 0 C[m][n] = sum_k A[m][k] B[n][k],
 * form 1 sum_k A[m][k] B[k][n], form 2 sum_k A[k][m] B[k][n]; epi 0 plain, 1 + bias[n], 2 relu(. + bias), 3 + res[m][ldc], 4 C +=.
 * fp32 matrices with row strides lda / ldb / ldc (elements); M % 4 == 0, N % 4 == 0, K % 16 == 0, A and B 16-byte aligned with
 * lda % 4 == ldb % 4 == 0.  Form 2 sums K in slices of 512 rows, added in slice order (the weight gradient's scheme); with more
 * than one slice the call takes a temporary buffer of the partial matrices from the device allocator and waits for `stream`. */
int vinet_token_gemm(int32_t mma, int32_t form, int32_t epi, const float* A, int32_t lda, const float* B, int32_t ldb,
                     float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, const float* res, void* stream);
/* split / mean / broadcast behind it (model.py:175-185).  x = tokens [B][Sv + n_audio][E], y [B][Sv positions][2E]:
 * y[b][pos][0:E] = x[b][pos], y[b][pos][E:2E] = mean over the n_audio last rows of x[b].  Backward writes (does not add)
 * dx: rows [0, Sv) = dy[..., 0:E]; each audio row = (1 / n_audio) * the sum of dy[..., E:2E] over positions in index order. */
int vinet_token_split_fwd(const VinetTensor* x, int32_t dtype, int32_t n_audio, const VinetTensor* y, void* stream);
int vinet_token_split_bwd(const VinetTensor* dy, int32_t dtype, int32_t n_audio, const VinetTensor* dx, void* stream);

/* ------------------------------------------------------------------------
 * Saliency-map post-processing: the host-side cv2 / torchvision steps of
 * generate_result.py:95-104 process() and train.py:251-253 validate(), on device.  Maps are dense float32
 * [B][H][W]; arithmetic follows opencv-python 3.4.3 / torchvision 0.5.0 (requirements.txt:96,178) as restated in
 * oracle/postproc_cpu.py, float32 without contraction.
 *
 * vinet_resize_blur: dst[b] = cv2.GaussianBlur(cv2.resize(src[b], (oW, oH)), (11, 11), 0)   (INTER_LINEAR; sigma 2.0,
 *   BORDER_REFLECT_101; utils.py:61-64 blur()).  `minmax` (optional, [B][2] words) receives the per-map minimum and
 *   maximum of dst as order-preserving keys -- opaque, for vinet_normalize_u8 only.
 * vinet_minmax: the same keys for maps that did not come out of vinet_resize_blur.
 * vinet_normalize_u8: utils.py:66-78 img_save(tensor, normalize=True) for each map on its own:
 *   x = (clamp(x, min, max) - min) / (max - min + 1e-5);  u8 = round_half_even(clamp(x * 255 + 0.5, 0, 255)).
 * ---------------------------------------------------------------------- */
int vinet_resize_blur(const float* src, int32_t B, int32_t H, int32_t W, float* dst, int32_t oH, int32_t oW,
                      uint32_t* minmax, void* stream);
int vinet_minmax(const float* src, int32_t B, int64_t n, uint32_t* minmax, void* stream);
int vinet_normalize_u8(const float* src, const uint32_t* minmax, int32_t B, int64_t n, uint8_t* dst, void* stream);

/* ------------------------------------------------------------------------
 * Input pipeline: decoded frames / ground-truth maps arrive as BYTES at their own
 * resolution and become the network's float32 inputs on device.  Scratch is the caller's (`*_ws_bytes`, 16-byte aligned).
 *
 * vinet_frames_preprocess: dataloader.py:243-250 / generate_result.py:77-88 img_transform --
 *   transforms.Resize((oH, oW)) [PIL Image.resize(BILINEAR): 22-bit fixed-point triangle filter, horizontal pass rounded
 *   to bytes, then vertical pass; Pillow pinned by requirements.txt:106] -> ToTensor (/ 255) -> Normalize.
 *   src uint8 [N][H][W][3] (RGB interleaved, = np.asarray(img.convert('RGB'))), dst float32 [N][3][oH][oW];
 *   mean_std: six HOST floats (mean r,g,b, std r,g,b), read during the call.
 * vinet_gt_preprocess: dataloader.py:283-296 -- uint8 'L' maps [N][H][W] -> float64 -> cv2.resize to (oW, oH) when the
 *   sizes differ (train mode; INTER_LINEAR, float32 weights, double arithmetic) -> / 255 when the map's maximum
 *   exceeds 1 -> float32 [N][oH][oW].
 * ---------------------------------------------------------------------- */
int64_t vinet_frames_preprocess_ws_bytes(int32_t N, int32_t H, int32_t W, int32_t oH, int32_t oW);
int vinet_frames_preprocess(const uint8_t* src, int32_t N, int32_t H, int32_t W, float* dst, int32_t oH, int32_t oW,
                            const float* mean_std, void* ws, void* stream);
/* vinet_audio_excerpt: dataloader.py:89-122 get_audio_feature -- out (win = 70560 floats) = zeros, with
 *   float(np.hanning(M)) * wav[start : end + 1] centred at win / 2 (offset win/2 - M/2; M = the clamped slice length;
 *   hanning in double with numpy 1.18.5's formula, requirements.txt:91).  wav is the device-resident waveform of the video
 *   (already scaled by 2^-23, dataloader.py:63). */
int vinet_audio_excerpt(const float* wav, int64_t n_samples, int64_t start, int64_t end, float* out, int32_t win, void* stream);
int64_t vinet_gt_preprocess_ws_bytes(int32_t N, int32_t oH, int32_t oW);
int vinet_gt_preprocess(const uint8_t* src, int32_t N, int32_t H, int32_t W, float* dst, int32_t oH, int32_t oW, void* ws,
                        void* stream);

/* misc */
/* Tuning / A-B switches (process-wide), `name` (default): meaning.  The list is vinet_amd/csrc/options.h, the one table the
 * library defines its switches from.  None of them changes results beyond floating-point accumulation order.
 * Returns 0; -1 for an unknown name.
 *   "dma" (1): LDS-DMA conv kernel (conv_dma) where legal; 0 = the register-staged kernel
 *   "dma3" (1): LDS-DMA kernel for the split-bf16 form (conv_dma3); 0 = the register-staged kernel
 *   "pp" (1): 256x256x64 ping-pong conv kernel: 0 off, 1 heuristic, 2 force, 3 / 4 force the 256- / 192-wide shape
 *   "pp_pw_kt" (8): ping-pong kernel on pointwise layers from this many K tiles of 64 (16 = as for every other layer)
 *   "pw" (1): pointwise streaming kernel (conv_pw) for 1x1x1 convs and their data gradients: 0 off, 1 heuristic, 2 also on
 *       small grids (tests)
 *   "pw_maxtn" (4): pointwise kernel: at most this many column tiles (each re-reads x)
 *   "ht" (1): halo-tile conv kernels (conv_ht): 0 off, 1 heuristic, 2 every eligible conv (tests)
 *   "ht3" (1): halo-tile kernels for the split-bf16 form; 0 = conv_dma3 everywhere
 *   "ht_minhw" (1344): halo tiles, spatial mode: smallest H x W the heuristic takes
 *   "ht_t" (1): temporal mode of the halo-tile kernel for (3,1,1) / stride-1 convs; 0 off
 *   "ht_t_minhw" (336): halo tiles, temporal mode: smallest H x W the heuristic takes
 *   "ht_pre" (0): halo tiles, spatial mode, on inputs with a pending BatchNorm + ReLU: 1 on
 *   "conv_hs" (1): strip-streaming kernel of the folded stem (conv_hs): 0 off, 1 heuristic, 2 every eligible shape (tests)
 *   "conv_hs_segs" (1): conv_hs: row segments for launches on small grids; 0 = whole strips only
 *   "conv_ts" (1): frame-streaming temporal 64 -> 64 kernels (conv_ts, conv_tsd): 0 off, 1 heuristic, 2 every eligible
 *       shape (tests)
 *   "conv_ts_segs" (1): conv_ts: frame segments for launches on small grids; 0 = whole patches only
 *   "splitk" (1): split-K on grids that cannot fill the chip: 0 off, 1 on, n >= 2 = minimum K chunks (of 32) per split
 *   "sk_tile" (7): tiles of long-K small-grid convs whose caller lends split-K scratch: bit 0 128x192, bit 1 128x128, bit
 *       2 / 3 128x64 / 256x64
 *   "n64_tile" (0): tuning: 64-wide layers on 128x64 (1) or 64x64 (2) tiles instead of 256x64
 *   "n64_kmax" (64): 64-wide outputs: 128-row tiles up to this many K steps of 32 (0 = never)
 *   "n128_tile" (0): tuning: 128-wide layers on 128x128 (1) or 64x128 (2) tiles instead of 256x128
 *   "n128_kmax" (64): 128-wide outputs: 128-row tiles up to this many K steps of 32 (0 = never)
 *   "n192_tile" (1): 128x192 tiles for N % 192 == 0 instead of 256x96: 0 off, 1 heuristic, 2 also on small grids (tests)
 *   "tperm" (0): t-fastest M-tile order (L2 reuse across temporal taps): 1 on
 *   "bnb_epi" (1): BatchNorm-backward partial sums out of the shared conv epilogue; 0 = only the fused temporal data
 *       gradient
 *   "wgrad_dma" (1): LDS-DMA multi-tap weight-gradient kernel where legal; 0 = the register-staged kernel
 *   "wgrad_tg" (0): tuning: taps per group in the LDS-DMA weight gradient (0 = heuristic)
 *   "wgrad_tr" (1): hardware transpose reads in the register-staged weight gradient; 0 = scalar LDS reads
 *   "wgrad_pp" (1): 256x256x64 ping-pong weight gradient: 0 off, 1 heuristic, 2 force, 3 / 4 force the 256- / 192-row tile
 *   "wgrad_pp_cap" (1): the ping-pong weight gradient honours VinetWgradDesc::max_cus; 0 = always the whole chip
 *   "wgrad_ts" (1): frame-streaming weight gradient of temporal 64 -> 64 convs: 0 off, 1 heuristic, 2 every eligible shape
 *       (tests)
 *   "wgrad_ts_cap" (0): the frame-streaming weight gradient honours VinetWgradDesc::max_cus: 1 on
 *   "wgrad_hs" (1): strip-streaming weight gradient of the folded stem: 0 off, 1 heuristic, 2 every eligible shape (tests)
 *   "wgrad_rs" (1): row-streaming weight gradient of 1x3x3 convs: 0 off, 1 heuristic, 2 every eligible shape (tests)
 *   "wgrad_rs4" (1): row-streaming weight gradient: the four-wave form for W = 24, 48, 32, 64, 96; 0 = the eight-wave
 *       kernels
 *   "wgrad_tf" (1): temporal-tap weight gradient (wgrad_tf): 0 off, 1 heuristic, 2 every eligible shape (tests)
 *   "wgrad_skinny" (1): weight gradient of pointwise convs with 8 output channels: 0 off, 1 heuristic, 2 every eligible
 *       shape (tests)
 *   "bn_lean" (1): register-lean bf16 BatchNorm-backward kernels: 0 = the generic 8-channel forms, 1 =
 *       register-lean
 *   "bn_rows" (1024): cap on the workgroups (= partial rows) of a channel reduction (clamped to >= 1)
 *   "reduce_il" (1): channel reductions: blocks interleave rounds over one window; 0 = one contiguous range per block
 *   "reduce_small" (1): tensors of <= 64 voxels take channel_reduce_small_kernel; 0 off
 *   "pack_tiled" (1): LDS-tiled multi-tensor pack / unpack; 0 = the element-wise kernels
 *   "pool_lds" (1): LDS halo-tile 3x3x3/s1 max-pool forward (C % 64 == 0): 0 off, 1 large tensors, 2 always
 *   "pool_pk" (1): bf16: packed 32-bit-key form of the LDS halo-tile pool; 0 = the fp32-compare kernel
 *   "pool_twalk" (1): T-walking 3x3x3/s1 max-pool backward: 0 off, 1 large tensors, 2 always (any value above 3 too), 3
 *       conditional-load form.  The forward's 8-channel T-walking kernel (kT 3, sT 1) reads it too: >= 2 forces it on
 *       small tensors, 0 does NOT switch it off
 *   "pool_blk" (1): strided max-pool backward per 2x2 input block; 0 off
 *   "up_blk" (1): 8-channel upsample kernels (forward per 2x2 output block); 0 off
 *   "auc_ws" (0): AUC-Judd sorts and counts in the caller's workspace whatever the number of fixations: 1 on (tests)
 *   "sauc_ws" (0): shuffled AUC reads the other-fixation list from the caller's workspace whatever its length: 1 on (tests) */
int vinet_set_option(const char* name, int32_t value);
/* fp32 view (with its pending affine applied) -> hi = bf16(v) and lo = bf16(v - hi) planes of the same dims: the operands of
 * the bf16 kernels when they serve the VINET_F32S arithmetic as three accumulating launches (hi*hi + lo*hi + hi*lo; the weight
 * gradients: every bf16 weight-gradient kernel ADDS into `dw`).  No reference counterpart: a numerics tool of this path. */
int vinet_split_bf16(const VinetTensor* src, VinetAffine pre, const VinetTensor* hi, const VinetTensor* lo, void* stream);
int vinet_fill_f32(float* p, int64_t n, float value, void* stream);
/* Test / tuning aid, no reference counterpart: one wave that idles for ~`cycles` shader clocks on `stream` (delays whatever is
 * enqueued behind it; touches no memory).  Used to perturb the two-stream backward schedule in eager mode. */
int vinet_debug_spin(int64_t cycles, void* stream);
int vinet_abi_version(void);
const char* vinet_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* VINET_HIP_H */
