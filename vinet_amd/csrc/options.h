// Every process-wide tuning / A-B switch of the library (vinet_set_option): VN_OPT(name, default, meaning and legal values).
// One line here is the whole of an option: common.h declares `g_vinet_opt_<name>` from this list for every translation unit,
// conv_api.hip defines the variables with these defaults and vinet_set_option looks names up in the same list.  The measured
// numbers behind a default live with the predicate that reads the switch.  None changes results beyond accumulation order.
#pragma once
#define VN_OPTIONS(VN_OPT) \
  VN_OPT(dma,          1, "LDS-DMA conv kernel (conv_dma) where legal; 0 = the register-staged kernel") \
  VN_OPT(dma3,         1, "LDS-DMA kernel for the split-bf16 form (conv_dma3); 0 = the register-staged kernel") \
  VN_OPT(pp,           1, "256x256x64 ping-pong conv kernel: 0 off, 1 heuristic, 2 force, 3 / 4 force the 256- / 192-wide shape") \
  VN_OPT(pp_pw_kt,     8, "ping-pong kernel on pointwise layers from this many K tiles of 64 (16 = as for every other layer)") \
  VN_OPT(pw,           1, "pointwise streaming kernel (conv_pw) for 1x1x1 convs and their data gradients: 0 off, 1 heuristic, 2 also on small grids (tests)") \
  VN_OPT(pw_maxtn,     4, "pointwise kernel: at most this many column tiles (each re-reads x)") \
  VN_OPT(ht,           1, "halo-tile conv kernels (conv_ht): 0 off, 1 heuristic, 2 every eligible conv (tests)") \
  VN_OPT(ht3,          1, "halo-tile kernels for the split-bf16 form; 0 = conv_dma3 everywhere") \
  VN_OPT(ht_minhw,     28 * 48, "halo tiles, spatial mode: smallest H x W the heuristic takes") \
  VN_OPT(ht_t,         1, "temporal mode of the halo-tile kernel for (3,1,1) / stride-1 convs; 0 off") \
  VN_OPT(ht_t_minhw,   14 * 24, "halo tiles, temporal mode: smallest H x W the heuristic takes") \
  VN_OPT(ht_pre,       0, "halo tiles, spatial mode, on inputs with a pending BatchNorm + ReLU: 1 on") \
  VN_OPT(conv_hs,      1, "strip-streaming kernel of the folded stem (conv_hs): 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(conv_hs_segs, 1, "conv_hs: row segments for launches on small grids; 0 = whole strips only") \
  VN_OPT(conv_ts,      1, "frame-streaming temporal 64 -> 64 kernels (conv_ts, conv_tsd): 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(conv_ts_segs, 1, "conv_ts: frame segments for launches on small grids; 0 = whole patches only") \
  VN_OPT(splitk,       1, "split-K on grids that cannot fill the chip: 0 off, 1 on, n >= 2 = minimum K chunks (of 32) per split") \
  VN_OPT(sk_tile,      7, "tiles of long-K small-grid convs whose caller lends split-K scratch: bit 0 128x192, bit 1 128x128, bit 2 / 3 128x64 / 256x64") \
  VN_OPT(n64_tile,     0, "tuning: 64-wide layers on 128x64 (1) or 64x64 (2) tiles instead of 256x64") \
  VN_OPT(n64_kmax,     64, "64-wide outputs: 128-row tiles up to this many K steps of 32 (0 = never)") \
  VN_OPT(n128_tile,    0, "tuning: 128-wide layers on 128x128 (1) or 64x128 (2) tiles instead of 256x128") \
  VN_OPT(n128_kmax,    64, "128-wide outputs: 128-row tiles up to this many K steps of 32 (0 = never)") \
  VN_OPT(n192_tile,    1, "128x192 tiles for N % 192 == 0 instead of 256x96: 0 off, 1 heuristic, 2 also on small grids (tests)") \
  VN_OPT(tperm,        0, "t-fastest M-tile order (L2 reuse across temporal taps): 1 on") \
  VN_OPT(bnb_epi,      1, "BatchNorm-backward partial sums out of the shared conv epilogue; 0 = only the fused temporal data gradient") \
  VN_OPT(wgrad_dma,    1, "LDS-DMA multi-tap weight-gradient kernel where legal; 0 = the register-staged kernel") \
  VN_OPT(wgrad_tg,     0, "tuning: taps per group in the LDS-DMA weight gradient (0 = heuristic)") \
  VN_OPT(wgrad_tr,     1, "hardware transpose reads in the register-staged weight gradient; 0 = scalar LDS reads") \
  VN_OPT(wgrad_pp,     1, "256x256x64 ping-pong weight gradient: 0 off, 1 heuristic, 2 force, 3 / 4 force the 256- / 192-row tile") \
  VN_OPT(wgrad_pp_cap, 1, "the ping-pong weight gradient honours VinetWgradDesc::max_cus; 0 = always the whole chip") \
  VN_OPT(wgrad_ts,     1, "frame-streaming weight gradient of temporal 64 -> 64 convs: 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(wgrad_ts_cap, 0, "the frame-streaming weight gradient honours VinetWgradDesc::max_cus: 1 on") \
  VN_OPT(wgrad_hs,     1, "strip-streaming weight gradient of the folded stem: 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(wgrad_rs,     1, "row-streaming weight gradient of 1x3x3 convs: 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(wgrad_rs4,    1, "row-streaming weight gradient: the four-wave form for W = 24, 48, 32, 64, 96; 0 = the eight-wave kernels") \
  VN_OPT(wgrad_tf,     1, "temporal-tap weight gradient (wgrad_tf): 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(wgrad_skinny, 1, "weight gradient of pointwise convs with 8 output channels: 0 off, 1 heuristic, 2 every eligible shape (tests)") \
  VN_OPT(bn_lean,      1, "register-lean bf16 BatchNorm-backward kernels: 0 = the generic 8-channel forms, 1 = register-lean") \
  VN_OPT(bn_rows,      1024, "cap on the workgroups (= partial rows) of a channel reduction (clamped to >= 1)") \
  VN_OPT(reduce_il,    1, "channel reductions: blocks interleave rounds over one window; 0 = one contiguous range per block") \
  VN_OPT(reduce_small, 1, "tensors of <= 64 voxels take channel_reduce_small_kernel; 0 off") \
  VN_OPT(pack_tiled,   1, "LDS-tiled multi-tensor pack / unpack; 0 = the element-wise kernels") \
  VN_OPT(pool_lds,     1, "LDS halo-tile 3x3x3/s1 max-pool forward (C % 64 == 0): 0 off, 1 large tensors, 2 always") \
  VN_OPT(pool_pk,      1, "bf16: packed 32-bit-key form of the LDS halo-tile pool; 0 = the fp32-compare kernel") \
  VN_OPT(pool_twalk,   1, "T-walking 3x3x3/s1 max-pool backward: 0 off, 1 large tensors, 2 always (any value above 3 too), 3 conditional-load form.  The forward's 8-channel T-walking kernel (kT 3, sT 1) reads it too: >= 2 forces it on small tensors, 0 does NOT switch it off") \
  VN_OPT(pool_blk,     1, "strided max-pool backward per 2x2 input block; 0 off") \
  VN_OPT(up_blk,       1, "8-channel upsample kernels (forward per 2x2 output block); 0 off") \
  VN_OPT(auc_ws,       0, "AUC-Judd sorts and counts in the caller's workspace whatever the number of fixations: 1 on (tests); 0 = in LDS up to 4096 fixations") \
  VN_OPT(sauc_ws,      0, "shuffled AUC reads the other-fixation list from the caller's workspace whatever its length: 1 on (tests); 0 = staged in LDS up to 8192 locations")

#define VN_OPT_DECLARE(name, dflt, text) extern int g_vinet_opt_##name;
VN_OPTIONS(VN_OPT_DECLARE)
