// Host-side functions of the convolution families that are defined in one translation unit and called from another (no kernel
// templates in here: the weight-gradient files include this header without conv_igemm.h), and the routing decision of a descriptor.
#pragma once
#include "common.h"

struct ConvArgs;
struct ConvTile { int MT, NT, WM, WN; int BM() const { return 16 * MT * WM; } int BN() const { return 16 * NT * WN; } };

// ---- which kernel a descriptor runs on: decided once, by vinet_conv_route / vinet_wgrad_route (conv_api.hip, conv_wgrad.hip) ----
enum ConvKind { CONV_TSD, CONV_HS, CONV_TS, CONV_PW, CONV_HT, CONV_PP, CONV_DMA, CONV_DMA3, CONV_IGEMM };
struct HtShape { int nt, tw, tm, pre, tilesH, tilesW; long tilesM; };   // column tile / 16, tile width, temporal mode, PRE form, spatial grid
struct PwShape { int nt, tilesN, gm, tpw; };
struct SplitK { int splits, per; long bytes; };
struct ConvRoute {
  ConvKind kind;
  bool tsd_ok;             // kind == CONV_TSD (tline == 3) only: the problem is eligible; else the launch refuses it
  ConvTile tile;           // CONV_DMA / CONV_IGEMM (and the M-tile order of fill_args)
  HtShape ht; PwShape pw;  // CONV_HT; CONV_PW
  int pp_bn, dma3_nt, segments;      // CONV_PP: column tile; CONV_DMA3: column tile / 16; CONV_HS / CONV_TS: row / frame segments per strip / patch
  SplitK splitk;           // CONV_DMA only: splits > 1 = the K loop is split (`query`: assuming scratch will be lent)
  int tile_m, stats_rows, bnb_rows, applies_pre_once;      // what the vinet_conv3d_* queries of the same names answer
};
ConvRoute vinet_conv_route(const VinetConvDesc* d, bool query);
enum WgradKind { WGRAD_SKINNY, WGRAD_RS, WGRAD_HS, WGRAD_TS, WGRAD_TF, WGRAD_PP, WGRAD_DMA, WGRAD_GENERIC };
struct WgradRoute { WgradKind kind; };
WgradRoute vinet_wgrad_route(const VinetWgradDesc* d);

// the tile is a pure function of (dtype, mode, M, N, K chunks, split-K scratch lent): callers size the statistics workspace by it
ConvTile vinet_pick_conv_tile(int dtype, int mode, long M, int N, long kchunks, bool may_split = false);
// conv_bf16.hip / conv_f32.hip / conv_bnb.hip: the template instantiations
int vinet_launch_conv_bf16(const ConvTile& t, int mode, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_f32(const ConvTile& t, int mode, const ConvArgs& a, hipStream_t s, bool split = false);
int vinet_launch_conv_dma_bf16(const ConvTile& t, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_dma_bnb(const ConvTile& t, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_dma3(int nt, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_pp_bf16(int bn, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_ht_bf16(int nt, int tw, int tm, int pre, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_ht_f32s(int nt, int tw, int tm, int pre, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_ht_bnb(int nt, int tw, int tm, const ConvArgs& a, hipStream_t s);
int vinet_launch_conv_pw_bf16(int nt, const ConvArgs& a, hipStream_t s);
// conv_hs.hip / conv_ts.hip: the stem's streaming kernels, eligibility next to the kernels
bool vinet_conv_use_hs(const VinetConvDesc* d);
int vinet_conv_hs_segments(const VinetConvDesc* d);
int vinet_launch_conv_hs(const VinetConvDesc* d, hipStream_t s);
bool vinet_conv_use_ts(const VinetConvDesc* d);
int vinet_conv_ts_positions(const VinetConvDesc* d);
int vinet_conv_ts_segments(const VinetConvDesc* d);
int vinet_launch_conv_ts(const VinetConvDesc* d, hipStream_t s);
bool vinet_conv_use_tsd(const VinetConvDesc* d);
int vinet_conv_tsd_bnb_rows(const VinetConvDesc* d);
int vinet_launch_conv_tsd(const VinetConvDesc* d, hipStream_t s);
// weight gradients: layout.hip (skinny), wgrad_rs / hs / ts / tf / pp / dma.hip
bool vinet_wgrad_use_skinny(const VinetWgradDesc* d);
int vinet_launch_wgrad_skinny(const VinetWgradDesc* d, hipStream_t s);
bool vinet_wgrad_use_rs(const VinetWgradDesc* d);
bool vinet_wgrad_rs_four_wave(const VinetWgradDesc* d);
int vinet_launch_wgrad_rs(const VinetWgradDesc* d, hipStream_t s);
bool vinet_wgrad_use_hs(const VinetWgradDesc* d);
int vinet_launch_wgrad_hs(const VinetWgradDesc* d, hipStream_t s);
bool vinet_wgrad_use_ts(const VinetWgradDesc* d);
int vinet_launch_wgrad_ts(const VinetWgradDesc* d, hipStream_t s);
bool vinet_wgrad_use_tf(const VinetWgradDesc* d);
int vinet_launch_wgrad_tf(const VinetWgradDesc* d, hipStream_t s);
bool vinet_wgrad_use_pp(const VinetWgradDesc* d);
int vinet_wgrad_pp_rows(int N);
int vinet_launch_wgrad_pp(const VinetWgradDesc* d, hipStream_t s);
int vinet_wgrad_dma_name(const VinetWgradDesc* d, char* buf, int n);
int vinet_launch_wgrad_dma(const VinetWgradDesc* d, hipStream_t s);
