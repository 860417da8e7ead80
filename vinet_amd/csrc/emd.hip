// Earth mover's distance (code_for_Metrics/EMD.m with FastEMD's emd_hat_gd_metric), the last metric of that folder.
//
// EMD.m: im1 = imresize(fixationMap, 1/downsize), im2 = imresize(saliencyMap, size(im1)), each divided by its sum, D = the
// Euclidean distance of the bin centres of the R x C grid, score = emd_hat_gd_metric(im1(:), im2(:), D, 0).  The double
// wrapper of that solver (emd_hat_impl.hpp:27-59, 396-475) pre-flows m = min(P, Q) per bin (p = P - m, q = Q - m: a bin is a
// source or a sink afterwards, never both; a negative bin of one map becomes demand on the other side), turns p, q and D into
// integers, ip = floor(p f + 0.5), iq = floor(q f + 0.5), iC = floor(D cf + 0.5) with f = 1e6 / max(sum P, sum Q) and
// cf = 1e6 / max D, makes the heavier side the supplier, and solves the integer transportation problem: every unit of the
// lighter side is shipped, the heavier side's surplus is dropped at no cost.  Its threshold node only re-routes arcs of cost
// max iC at the same cost and its artificial node is never in an optimum, so the minimum K over the dense bipartite graph is
// the solver's value, and score = K / f / cf.  K <= 1e12 is exact in int64.
//
// Three kernels, one workgroup (256 lanes) per map:
//   emd_prepare_kernel   the two separable resizes from the host's fp64 weight matrices, the sums, the division, then
//                        emd_quantise: pre-flow, the integers, f and the swap flag into the workspace;
//   emd_hist_kernel      the same emd_quantise on histograms the caller hands over (vinet_emd_hist);
//   emd_solve_kernel     K by successive shortest paths with node potentials, below.
// Every fp64 sum runs in a fixed order inside one workgroup and everything after the quantisation is integer arithmetic: a
// map's score and cost are the same bits alone and inside any batch.  All floating point is scalar fp64 (-ffp-contract=off: the
// products p * f + 0.5 are not fused, as the reference's are not).
//
// The solver.  Nodes are the S bins with supply and the T bins with demand, S + T = n <= R C.  iC depends on (|dr|, |dc|) alone:
// an R x C int32 table in LDS, never an n x n matrix.  Forward arcs source -> sink have no capacity; the reverse arc sink j ->
// source i has the residual capacity flow(i, j).  The flow is a dense int32 matrix [T][S] in the workspace, sink-major, so that
// the reverse arcs of one sink are one contiguous row.  Potentials pi (int64) keep every residual arc's reduced cost
// c(u, v) + pi(u) - pi(v) >= 0, so each augmenting path comes from one Dijkstra run that starts at every source with supply
// left and ends when the node it takes off the front is a sink with demand left.  One Dijkstra round: a workgroup arg-min over
// the unscanned nodes (wave shuffles, then four LDS slots, double-buffered by the round's parity: one barrier per round),
// ties to the smaller node number, then every lane relaxes the arcs from that node to the nodes it owns (node v belongs to lane
// v % 256: dist, parent and the scanned flag of a node are only ever touched by its lane).  Lane 0 walks the parents back to the
// root, takes the bottleneck and updates the flow; pi(v) += dist(v) - dist(target) for the scanned nodes.
//
// Loop bounds (all static, from n = S + T):
//   * a Dijkstra run scans a node per round and there are n nodes: at most n + 1 rounds;
//   * a path visits a node once: the walk to the root takes at most n steps;
//   * an augmentation (i) exhausts a source, (ii) fills a sink, or (iii) empties a reverse arc on its path.  (i) and (ii)
//     happen at most S + T times in total.  (iii) has no such bound: successive shortest paths is pseudo-polynomial, the only
//     general bound is one unit per augmentation, 1e6 + n.  On random dense histograms the host model counts 1.1 to 2.1 n
//     augmentations (12x20: 442 for n = 240; 16x32: 1043 for n = 510).  The kernel allows EMD_AUG_FACTOR * n + 16 = 16 n + 16,
//     eight times that, and a map that gets there receives NaN and status 1 instead of an answer: the guard bounds the
//     kernel at (16 n + 16)(n + 1) rounds, 4.2 million for n = 512, a few seconds, whatever the input.
// EMD_MAX_BINS = 512 (a 512 x 1024 map at downsize 32, 1080 x 1920 at 64): the per-node state is 36 bytes and the table 4 per bin,
// 20 KB of LDS per workgroup, so LDS is not what limits it; the flow matrix (n/2)^2 x 4 B = 256 KB per map and the cubic round
// bound are.  vinet_emd refuses more bins before any launch.
#include <math.h>

#include "common.h"

#define EMD_LANES 256
#define EMD_WAVES (EMD_LANES / 64)
#define EMD_MAX_BINS 512
#define EMD_TILE 1024
#define EMD_AUG_FACTOR 16
#define EMD_INF (1ll << 60)
#define EMD_MULT 1000000.0

enum { EMD_OK = 0, EMD_AUG_CAP = 1, EMD_NO_PATH = 2, EMD_BAD_PATH = 3, EMD_MASS_RANGE = 4 };

struct EmdHead {
  double f;              // 1e6 / max(sum P, sum Q)
  long long tot_p, tot_q;
  int32_t swap;          // sum iq > sum ip: Q supplies
  int32_t nan;           // the score is NaN: a sum is zero or not finite, or the grid has one bin
};

static size_t emd_flow_entries(int N) { return (size_t)(N / 2) * (size_t)((N + 1) / 2); }          // max S T with S + T <= N
static size_t emd_ws_per_map(int N) { return sizeof(EmdHead) + 2 * (size_t)N * sizeof(long long) + vn_pad8(emd_flow_entries(N) * 4); }

VN_DEV long long emd_block_sum_ll(long long v, long long* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = 0;
  for (int k = 0; k < EMD_WAVES; ++k) r += sh[k];
  return r;
}

// P, Q: N doubles each (LDS or global), read by every lane.  Writes the head, ip [N] and iq [N].
VN_DEV void emd_quantise(const double* P, const double* Q, int N, int one_bin, EmdHead* head, long long* ip, long long* iq, double* shd,
                         long long* shl) {
  const int tid = threadIdx.x;
  if (tid == 0) {          // the reference's order: one running sum each, bin after bin
    double sp = 0.0, sq = 0.0;
    for (int i = 0; i < N; ++i) { sp += P[i]; sq += Q[i]; }
    shd[0] = sp; shd[1] = sq;
  }
  __syncthreads();
  const double sp = shd[0], sq = shd[1];
  const double big = sp > sq ? sp : sq;
  const bool bad = one_bin || !(big > 0.0) || !(fabs(sp) < INFINITY) || !(fabs(sq) < INFINITY);
  const double f = EMD_MULT / big;
  long long tp = 0, tq = 0;
  for (int i = tid; i < N; i += EMD_LANES) {
    long long a = 0, b = 0;
    if (!bad) {
      const double p = P[i], q = Q[i];
      const double m = p < q ? p : q;
      a = (long long)floor((p - m) * f + 0.5);
      b = (long long)floor((q - m) * f + 0.5);
    }
    ip[i] = a; iq[i] = b;
    tp += a; tq += b;
  }
  tp = emd_block_sum_ll(tp, shl);
  tq = emd_block_sum_ll(tq, shl);
  if (tid == 0) {
    head->f = f; head->tot_p = tp; head->tot_q = tq;
    head->swap = tq > tp ? 1 : 0;
    head->nan = bad ? 1 : 0;
  }
}

// one separable resize into out [R][C] (LDS): out[r][c] = sum_w Wc[c][w] * (sum_h Wr[r][h] * x[h][w]), h and w ascending, zero
// weights skipped (imresize keeps the non-zero taps only)
VN_DEV void emd_resize(const void* x, int is64, int H, int W, const double* __restrict__ Wr, const double* __restrict__ Wc, int R, int C,
                       double* out, double* tile, long off) {
  const int tid = threadIdx.x;
  for (int i = tid; i < R * C; i += EMD_LANES) out[i] = 0.0;
  for (int r = 0; r < R; ++r)
    for (int w0 = 0; w0 < W; w0 += EMD_TILE) {
      double acc[EMD_TILE / EMD_LANES];
#pragma unroll
      for (int k = 0; k < EMD_TILE / EMD_LANES; ++k) acc[k] = 0.0;
      for (int h = 0; h < H; ++h) {
        const double wt = Wr[(long)r * H + h];
        if (wt == 0.0) continue;
#pragma unroll
        for (int k = 0; k < EMD_TILE / EMD_LANES; ++k) {
          const int w = w0 + tid + k * EMD_LANES;
          if (w < W) acc[k] += wt * ldg_rt(x, is64, off + (long)h * W + w);
        }
      }
      __syncthreads();          // the tile's readers of the pass before are done
#pragma unroll
      for (int k = 0; k < EMD_TILE / EMD_LANES; ++k) tile[tid + k * EMD_LANES] = acc[k];
      __syncthreads();
      const int tw = W - w0 < EMD_TILE ? W - w0 : EMD_TILE;
      for (int c = tid; c < C; c += EMD_LANES) {
        double a = out[r * C + c];
        const double* wc = Wc + (long)c * W + w0;
        for (int wl = 0; wl < tw; ++wl) {
          const double wt = wc[wl];
          if (wt != 0.0) a += wt * tile[wl];
        }
        out[r * C + c] = a;
      }
    }
  __syncthreads();
}

__global__ __launch_bounds__(EMD_LANES) void emd_prepare_kernel(const void* __restrict__ s, int s64, int Hs, int Ws, const void* __restrict__ gt,
                                                                int g64, int Hg, int Wg, int R, int C, const double* __restrict__ wgr,
                                                                const double* __restrict__ wgc, const double* __restrict__ wsr,
                                                                const double* __restrict__ wsc, char* ws, size_t per_map,
                                                                double* __restrict__ hist_out) {
  __shared__ double tile[EMD_TILE];
  __shared__ double hp[EMD_MAX_BINS], hq[EMD_MAX_BINS];
  __shared__ double shd[2];
  __shared__ long long shl[EMD_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, N = R * C;
  emd_resize(gt, g64, Hg, Wg, wgr, wgc, R, C, hp, tile, (long)b * Hg * Wg);
  emd_resize(s, s64, Hs, Ws, wsr, wsc, R, C, hq, tile, (long)b * Hs * Ws);
  if (tid == 0) {
    double sp = 0.0, sq = 0.0;
    for (int i = 0; i < N; ++i) { sp += hp[i]; sq += hq[i]; }
    shd[0] = sp; shd[1] = sq;
  }
  __syncthreads();
  const double sp = shd[0], sq = shd[1];
  for (int i = tid; i < N; i += EMD_LANES) {
    hp[i] = hp[i] / sp;
    hq[i] = hq[i] / sq;
    if (hist_out) {
      hist_out[((long)b * 2) * N + i] = hp[i];
      hist_out[((long)b * 2 + 1) * N + i] = hq[i];
    }
  }
  __syncthreads();
  char* w = ws + (size_t)b * per_map;
  emd_quantise(hp, hq, N, N == 1, (EmdHead*)w, (long long*)(w + sizeof(EmdHead)), (long long*)(w + sizeof(EmdHead)) + N, shd, shl);
}

__global__ __launch_bounds__(EMD_LANES) void emd_hist_kernel(const double* __restrict__ P, const double* __restrict__ Q, int N, int one_bin,
                                                             char* ws, size_t per_map) {
  __shared__ double shd[2];
  __shared__ long long shl[EMD_WAVES];
  const int b = blockIdx.x;
  char* w = ws + (size_t)b * per_map;
  emd_quantise(P + (long)b * N, Q + (long)b * N, N, one_bin, (EmdHead*)w, (long long*)(w + sizeof(EmdHead)),
               (long long*)(w + sizeof(EmdHead)) + N, shd, shl);
}

__global__ __launch_bounds__(EMD_LANES) void emd_solve_kernel(int R, int C, char* ws, size_t per_map, double* __restrict__ score,
                                                              long long* __restrict__ cost, int* __restrict__ status) {
  __shared__ long long dist[EMD_MAX_BINS], pi[EMD_MAX_BINS];
  __shared__ int rem[EMD_MAX_BINS], rc[EMD_MAX_BINS], par[EMD_MAX_BINS], scanned[EMD_MAX_BINS], ctab[EMD_MAX_BINS];
  __shared__ long long slot_v[2][EMD_WAVES], shl[EMD_WAVES];
  __shared__ int slot_i[2][EMD_WAVES];
  __shared__ int sh_S, sh_T, sh_status;
  __shared__ long long sh_left;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, N = R * C;
  char* w = ws + (size_t)b * per_map;
  const EmdHead* head = (const EmdHead*)w;
  const long long* ip = (const long long*)(w + sizeof(EmdHead));
  const long long* iq = ip + N;
  int* flow = (int*)(w + sizeof(EmdHead) + 2 * (size_t)N * sizeof(long long));          // [T][S]
  const double maxd = sqrt((double)((R - 1) * (R - 1) + (C - 1) * (C - 1)));
  const double cf = EMD_MULT / maxd;
  const int swap = head->swap;
  const long long tot_sup = swap ? head->tot_q : head->tot_p, tot_dem = swap ? head->tot_p : head->tot_q;
  if (head->nan || tot_sup > 0x7fffffffll) {          // (uniform: the head is the same for every lane)
    if (tid == 0) {
      score[b] = NAN;
      if (cost) cost[b] = 0;
      if (status) status[b] = head->nan ? EMD_OK : EMD_MASS_RANGE;
    }
    return;
  }
  for (int i = tid; i < N; i += EMD_LANES) {
    const int dr = i / C, dc = i - dr * C;
    ctab[i] = (int)(long long)floor(sqrt((double)(dr * dr + dc * dc)) * cf + 0.5);
  }
  if (tid == 0) {          // the nodes: sources then sinks, each side in bin order (N <= 512: a serial pass)
    const long long* sup = swap ? iq : ip;
    const long long* dem = swap ? ip : iq;
    int S = 0, T = 0;
    for (int i = 0; i < N; ++i)
      if (sup[i] > 0) { rem[S] = (int)sup[i]; rc[S] = ((i / C) << 16) | (i % C); ++S; }
    for (int i = 0; i < N; ++i)
      if (dem[i] > 0 && S + T < EMD_MAX_BINS) { rem[S + T] = (int)dem[i]; rc[S + T] = ((i / C) << 16) | (i % C); ++T; }
    sh_S = S; sh_T = T; sh_status = EMD_OK; sh_left = tot_dem;
  }
  __syncthreads();
  const int S = sh_S, T = sh_T, n = S + T;
  for (int i = tid; i < S * T; i += EMD_LANES) flow[i] = 0;
  for (int v = tid; v < n; v += EMD_LANES) pi[v] = 0;
  __syncthreads();
#define EMD_COST(a, z) ctab[abs((rc[a] >> 16) - (rc[z] >> 16)) * C + abs((rc[a] & 0xffff) - (rc[z] & 0xffff))]
  const int aug_cap = EMD_AUG_FACTOR * n + 16;
  int st = EMD_OK;
  for (int aug = 0; aug < aug_cap && sh_left > 0; ++aug) {
    for (int v = tid; v < n; v += EMD_LANES) {
      dist[v] = (v < S && rem[v] > 0) ? 0 : EMD_INF;
      par[v] = -1;
      scanned[v] = 0;
    }
    int target = -1;
    long long dt = 0;
    for (int round = 0; round <= n; ++round) {
      long long best = EMD_INF;
      int bi = 0x7fffffff;
      for (int v = tid; v < n; v += EMD_LANES)
        if (!scanned[v] && dist[v] < best) { best = dist[v]; bi = v; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const long long ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      const int sl = round & 1;
      if (lane == 0) { slot_v[sl][wv] = best; slot_i[sl][wv] = bi; }
      __syncthreads();
      best = slot_v[sl][0]; bi = slot_i[sl][0];
#pragma unroll
      for (int k = 1; k < EMD_WAVES; ++k) {
        const long long ob = slot_v[sl][k];
        const int oi = slot_i[sl][k];
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (best >= EMD_INF) { st = EMD_NO_PATH; break; }
      const int u = bi;
      if (u >= S && rem[u] > 0) { target = u; dt = best; break; }
      if ((u & (EMD_LANES - 1)) == tid) scanned[u] = 1;
      const long long base = best + pi[u];
      if (u < S) {
        for (int j = tid; j < n; j += EMD_LANES)
          if (j >= S && !scanned[j]) {
            const long long nd = base + EMD_COST(u, j) - pi[j];
            if (nd < dist[j]) { dist[j] = nd; par[j] = u; }
          }
      } else {
        const int* row = flow + (size_t)(u - S) * S;
        for (int i = tid; i < S; i += EMD_LANES)
          if (!scanned[i] && row[i] > 0) {
            const long long nd = base - EMD_COST(i, u) - pi[i];
            if (nd < dist[i]) { dist[i] = nd; par[i] = u; }
          }
      }
    }
    if (st == EMD_OK && target < 0) st = EMD_BAD_PATH;          // (n + 1 rounds without a target: cannot happen, n nodes)
    if (st != EMD_OK) break;
    for (int v = tid; v < n; v += EMD_LANES)
      if (scanned[v]) pi[v] += dist[v] - dt;
    __syncthreads();
    if (tid == 0) {
      int v = target, steps = 0, amt = rem[target];
      while (par[v] >= 0 && steps <= n) {
        const int p = par[v];
        if (v < S) { const int f = flow[(size_t)(p - S) * S + v]; amt = f < amt ? f : amt; }
        v = p; ++steps;
      }
      if (steps > n || v >= S || rem[v] <= 0) sh_status = EMD_BAD_PATH;
      else {
        amt = rem[v] < amt ? rem[v] : amt;
        if (amt <= 0) sh_status = EMD_BAD_PATH;
        else {
          rem[v] -= amt; rem[target] -= amt; sh_left -= amt;
          v = target;
          while (par[v] >= 0) {
            const int p = par[v];
            if (v < S) flow[(size_t)(p - S) * S + v] -= amt;
            else flow[(size_t)(v - S) * S + p] += amt;
            v = p;
          }
        }
      }
    }
    __syncthreads();
    if (sh_status != EMD_OK) { st = sh_status; break; }
  }
  __syncthreads();
  if (st == EMD_OK && sh_left > 0) st = EMD_AUG_CAP;
  long long K = 0;
  if (st == EMD_OK)
    for (int e = tid; e < S * T; e += EMD_LANES) {
      const int j = e / S, i = e - j * S;
      K += (long long)flow[e] * EMD_COST(i, S + j);
    }
  K = emd_block_sum_ll(K, shl);
#undef EMD_COST
  if (tid == 0) {
    score[b] = st == EMD_OK ? (double)K / head->f / cf : NAN;
    if (cost) cost[b] = st == EMD_OK ? K : -1;
    if (status) status[b] = st;
  }
}

static int emd_check_grid(const char* who, int32_t B, int32_t R, int32_t C) {
  VN_CHECK_ARG(B > 0, "%s: B must be positive", who);
  VN_CHECK_ARG(R >= 1 && C >= 1, "%s: the grid needs at least one bin (R %d, C %d)", who, R, C);
  VN_CHECK_ARG((long)R * C <= EMD_MAX_BINS, "%s: %d x %d = %ld bins, more than the %d this solver takes (use a larger downsize)", who, R, C,
               (long)R * C, EMD_MAX_BINS);
  return 0;
}

extern "C" size_t vinet_emd_workspace(int32_t B, int32_t R, int32_t C) {
  if (B <= 0 || R < 1 || C < 1 || (long)R * C > EMD_MAX_BINS) return 0;
  return (size_t)B * emd_ws_per_map(R * C);
}

static int emd_check_ws(const char* who, int32_t B, int32_t R, int32_t C, const void* workspace, size_t workspace_bytes) {
  const size_t need = vinet_emd_workspace(B, R, C);
  VN_CHECK_ARG(workspace && workspace_bytes >= need && (((uintptr_t)workspace) & 7) == 0,
               "%s: workspace of %zu bytes (8-byte aligned) needed, got %zu", who, need, workspace ? workspace_bytes : (size_t)0);
  return 0;
}

extern "C" int vinet_emd(const void* s, int32_t s_is_f64, int32_t Hs, int32_t Ws, const void* gt, int32_t gt_is_f64, int32_t Hg, int32_t Wg,
                         int32_t B, int32_t downsize, int32_t R, int32_t C, const double* w_gt_r, const double* w_gt_c, const double* w_s_r,
                         const double* w_s_c, void* workspace, size_t workspace_bytes, double* score, int64_t* cost, int32_t* status,
                         double* hist_out, void* stream) {
  VN_CHECK_ARG(downsize >= 1, "emd: downsize must be at least 1, got %d", downsize);
  if (emd_check_grid("emd", B, R, C)) return -1;
  VN_CHECK_ARG(Hs > 0 && Ws > 0 && Hg > 0 && Wg > 0 && (long)Hs * Ws <= (1l << 30) && (long)Hg * Wg <= (1l << 30),
               "emd: map sizes must be positive (at most 2^30 pixels)");
  VN_CHECK_ARG(R == (Hg + downsize - 1) / downsize && C == (Wg + downsize - 1) / downsize,
               "emd: a %d x %d ground truth at downsize %d has %d x %d bins, not %d x %d", Hg, Wg, downsize, (Hg + downsize - 1) / downsize,
               (Wg + downsize - 1) / downsize, R, C);
  VN_CHECK_ARG(s && gt && score && w_gt_r && w_gt_c && w_s_r && w_s_c, "emd: null map, weight matrix or score");
  if (emd_check_ws("emd", B, R, C, workspace, workspace_bytes)) return -1;
  const size_t per = emd_ws_per_map(R * C);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(emd_prepare_kernel, dim3(B), dim3(EMD_LANES), 0, st, s, s_is_f64 ? 1 : 0, Hs, Ws, gt, gt_is_f64 ? 1 : 0, Hg, Wg, R, C,
                     w_gt_r, w_gt_c, w_s_r, w_s_c, (char*)workspace, per, hist_out);
  hipLaunchKernelGGL(emd_solve_kernel, dim3(B), dim3(EMD_LANES), 0, st, R, C, (char*)workspace, per, score, (long long*)cost, status);
  return vn_launch_status("emd");
}

extern "C" int vinet_emd_hist(const double* P, const double* Q, int32_t B, int32_t R, int32_t C, void* workspace, size_t workspace_bytes,
                              double* score, int64_t* cost, int32_t* status, void* stream) {
  if (emd_check_grid("emd_hist", B, R, C)) return -1;
  VN_CHECK_ARG(P && Q && score, "emd_hist: null histogram or score");
  if (emd_check_ws("emd_hist", B, R, C, workspace, workspace_bytes)) return -1;
  const size_t per = emd_ws_per_map(R * C);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(emd_hist_kernel, dim3(B), dim3(EMD_LANES), 0, st, P, Q, R * C, R * C == 1 ? 1 : 0, (char*)workspace, per);
  hipLaunchKernelGGL(emd_solve_kernel, dim3(B), dim3(EMD_LANES), 0, st, R, C, (char*)workspace, per, score, (long long*)cost, status);
  return vn_launch_status("emd_hist");
}
