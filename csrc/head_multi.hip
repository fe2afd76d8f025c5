// 1x1 output head for K classes (64 -> K, with bias, 2 <= K <= 8) fused with softmax cross-entropy,
// and its serving form (class-selected mask). The one-class head lives in head_loss.hip.
//
// Reference: OutConv = nn.Conv2d(64, n_classes, 1); loss = F.cross_entropy(logits, labels,
// ignore_index=255), mean over the kept pixels.
//
// headk_fwd: logits[p][k] = sum_c a[p][c]*w[k][c] + b[k] (pixel-major fp32); per-block partials of
//   {sum ce, kept pixels}, ce = logsumexp(x) - x[label] with the max subtracted.
//   Labels are uint8; 255 is ignored, and so is every label >= K (never used as an index).
//   headk_loss_finalize: sums = {sum ce, count}, loss = sum ce / max(count, 1) (fp64 sum).
//   If every pixel is ignored the loss is 0 and every gradient is 0 (torch returns NaN there).
// headk_bwd: dlogit[k] = (softmax(x)[k] - [k == label]) * gscale / count for kept pixels, 0 for
//   ignored ones (count read from `sums` on the device); da[p][c] = bf16(sum_k dlogit[k]*w[k][c]);
//   per-block partials [blk][K*64 + K] of dW and db; headk_grad_finalize sums them into the gradient
//   views in the parameter's [K][64] order.
// headk_mask: mask[p] = argmax_k(a[p].w[k] + b[k]) == cls, ties to the lowest index.
//
// Extended mode (EXT; class weights cw[k] >= 0 and / or a soft Dice term of weight dice_w; the plain
// kernels above are the EXT = false instantiations and are not touched by it). s = softmax(x):
//   W = sum_kept cw[t], CE = sum_kept cw[t] * ce / W (0 if W == 0; F.cross_entropy(weight=cw)),
//   I_k = sum_kept s_k [t == k], P_k = sum_kept s_k, T_k = sum_kept [t == k], D_k = P_k + T_k + eps,
//   Dice = 1 - (1/K) sum_k (2 I_k + eps) / D_k over the whole batch, loss[0] = CE + dice_w * Dice,
//   loss[1] = CE. The weights act on CE only.
// headk_fwd: per-block partial rows of 2 + 3K floats {sum cw*ce, sum cw, I_0.., P_0.., T_0..}; after
//   the max / sum-exp shuffles lane `sub < K` owns s_k, so I / P / T accumulate in the owning lane.
//   headk_loss_finalize_ext: sums[0 .. 2+3K) = {sum cw*ce, W, I_k, P_k, T_k} (fp64 sums).
// headk_bwd: dlogit[j] = cw[t] (s_j - [j == t]) / W + s_j (G_j - sum_k G_k s_k) with
//   G_k = B_k + [t == k] A_k, A_k = -2 dice_w / (K D_k), B_k = dice_w (2 I_k + eps) / (K D_k^2),
//   formed once per thread from `sums`; the rest is the plain backward.
//
// Memory pattern of head_loss.hip: 8 lanes per pixel, one 16-B load of 8 bf16 channels per lane,
// HPX pixels in flight per lane group, grid capped at 2048 blocks, per-block partial rows and a
// one-launch finalize. No float atomics: results are bitwise repeatable.
//
// The K per-lane partial dots of a pixel are reduced over its 8 lanes transpose-style: at each step
// a lane keeps one half of its values and hands the other half to its partner, so after log2(KP)
// steps (KP = K rounded up to a power of two) lane `sub` owns logit `sub & (KP - 1)` -- 7 shuffles
// at K = 8 where K separate butterflies would take 24.
#include "common.h"
#include "head_multi_dev.h"
#include "rdp_api.h"
#include <algorithm>

#define HEAD_C 64
#define HPX 4  // pixels in flight per 8-lane group

namespace {

// pow2_classes, reduce_transpose, lane_logit, argmax_lowest: shared with the row-ring conv's fused
// K-class head, which must reproduce headk_mask_kernel's bits (head_multi_dev.h)
using namespace rdp_headk;

// EXT: `cw` = class weights (null: all 1); partial rows of 2 + 3K floats instead of 2
template <int K, bool EXT>
__global__ __launch_bounds__(256) void headk_fwd_kernel(const u16* __restrict__ a, int apitch,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        const uint8_t* __restrict__ labels,
                                                        float* __restrict__ logits, float* __restrict__ partial,
                                                        int M, const float* __restrict__ cw) {
  constexpr int KP = pow2_classes(K);
  constexpr int PROW = EXT ? 2 + 3 * K : 2;
  __shared__ float red[4][PROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & 7;
  const int kk = sub & (KP - 1);  // the logit this lane ends up owning
  const bool own = kk < K;
  float wl[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) wl[k][j] = w[k * HEAD_C + sub * 8 + j];
  const float bias = own ? b[kk] : 0.f;
  float sce = 0.f, scnt = 0.f;
  // EXT: the weight of the class this lane owns; softmax sums of that class over the kept pixels
  [[maybe_unused]] float wk = 1.f, accI = 0.f, accP = 0.f, accT = 0.f;
  if constexpr (EXT) {
    if (cw != nullptr && sub < K) wk = cw[sub];
  }
  const long stride = (long)gridDim.x * 32;  // 32 pixel groups per block
  for (long p0 = blockIdx.x * 32l + (threadIdx.x >> 3); p0 < M; p0 += stride * HPX) {
    uint4 v[HPX];
    int lab[HPX];
#pragma unroll
    for (int u = 0; u < HPX; ++u) {
      const long p = p0 + u * stride;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      lab[u] = 255;
      if (p < M) {
        v[u] = *(const uint4*)(a + (size_t)p * apitch + sub * 8);
        lab[u] = labels[p];
      }
    }
#pragma unroll
    for (int u = 0; u < HPX; ++u) {  // every lane runs the shuffles (zeros past M); only stores are guarded
      const long p = p0 + u * stride;
      float f[8];
      unpack8(v[u], f);
      const float x = lane_logit<K>(f, wl, sub) + bias;
      float mx = own ? x : -INFINITY;
#pragma unroll
      for (int o = 1; o < KP; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float se = own ? __expf(x - mx) : 0.f;
      [[maybe_unused]] const float ex = se;  // this lane's own exp(x - max)
#pragma unroll
      for (int o = 1; o < KP; o <<= 1) se += __shfl_xor(se, o, 64);
      if (p < M) {
        if (sub < K) logits[(size_t)p * K + sub] = x;  // sub < K: kk == sub
        if constexpr (EXT) {
          if (lab[u] < K && sub < K) {  // kept pixel: every class lane adds its softmax value
            const float sp = ex / se;
            accP += sp;
            if (sub == lab[u]) {
              accI += sp;
              accT += 1.f;
              sce += wk * (mx + logf(se) - x);
              scnt += wk;
            }
          }
        } else {
          if (lab[u] < K && sub == lab[u]) {  // kept pixel: the lane that owns x[label] finishes it
            sce += mx + logf(se) - x;
            scnt += 1.f;
          }
        }
      }
    }
  }
  sce = wave_sum(sce);
  scnt = wave_sum(scnt);
  if (lane == 0) { red[wave][0] = sce; red[wave][1] = scnt; }
  if constexpr (EXT) {
    // the 8 pixel groups of the wave share `sub`: after three steps lanes 0..7 hold class `lane`'s totals
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      accI += __shfl_xor(accI, o, 64);
      accP += __shfl_xor(accP, o, 64);
      accT += __shfl_xor(accT, o, 64);
    }
    if (lane < K) {
      red[wave][2 + lane] = accI;
      red[wave][2 + K + lane] = accP;
      red[wave][2 + 2 * K + lane] = accT;
    }
  }
  __syncthreads();
  if (threadIdx.x < PROW) {
    const int q = threadIdx.x;
    partial[blockIdx.x * PROW + q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
  }
}

// sums[0..1] = {sum ce, kept pixels}; loss[0] = loss[1] = mean ce over the kept pixels (0 if none)
__global__ void headk_loss_finalize_kernel(const float* __restrict__ partial, int T, float* __restrict__ sums,
                                           float* __restrict__ loss) {
  __shared__ double red[2][64];
  const int q = threadIdx.x >> 6, l = threadIdx.x & 63;  // 128 threads: 2 quantities x 64 lanes
  double s = 0.0;
  for (int t = l; t < T; t += 64) s += (double)partial[t * 2 + q];
  red[q][l] = s;
  __syncthreads();
  if (threadIdx.x < 2) {
    double tot = 0.0;
    for (int k = 0; k < 64; ++k) tot += red[threadIdx.x][k];
    sums[threadIdx.x] = (float)tot;
    red[threadIdx.x][0] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = red[1][0] > 1.0 ? red[1][0] : 1.0;
    const float L = (float)(red[0][0] / cnt);
    loss[0] = L;
    loss[1] = L;
  }
}

// EXT: sums[0 .. 2+3K) = {sum cw*ce, W, I_k, P_k, T_k} from partial rows of n = 2 + 3K floats, each summed
// in the order of the plain finalize; loss[0] = CE + dice_w * Dice, loss[1] = CE = sum cw*ce / W (0 if
// W == 0: W may be below 1 with small weights, so there is no max(W, 1) here)
__global__ __launch_bounds__(256) void headk_loss_finalize_ext_kernel(const float* __restrict__ partial, int T,
                                                                      int K, float dice_w, float dice_eps,
                                                                      float* __restrict__ sums,
                                                                      float* __restrict__ loss) {
  constexpr int NMAX = 2 + 3 * 8;
  __shared__ double red[NMAX][64];
  __shared__ double tot[NMAX];
  const int n = 2 + 3 * K;
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int q = wave; q < n; q += 4) {
    double s = 0.0;
    for (int t = l; t < T; t += 64) s += (double)partial[t * n + q];
    red[q][l] = s;
  }
  __syncthreads();
  if (threadIdx.x < n) {
    double v = 0.0;
    for (int k = 0; k < 64; ++k) v += red[threadIdx.x][k];
    sums[threadIdx.x] = (float)v;
    tot[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ce = tot[1] > 0.0 ? tot[0] / tot[1] : 0.0;
    double ratio = 0.0;
    for (int k = 0; k < K; ++k)
      ratio += (2.0 * tot[2 + k] + (double)dice_eps) / (tot[2 + K + k] + tot[2 + 2 * K + k] + (double)dice_eps);
    const double dice = 1.0 - ratio / K;
    loss[0] = (float)(ce + (double)dice_w * dice);
    loss[1] = (float)ce;
  }
}

template <int K, bool EXT>
__global__ __launch_bounds__(256) void headk_bwd_kernel(const u16* __restrict__ a, int apitch,
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ logits,
                                                        const uint8_t* __restrict__ labels,
                                                        const float* __restrict__ sums, u16* __restrict__ da,
                                                        int dapitch, float* __restrict__ partial, int M,
                                                        float gscale, const float* __restrict__ cw, float dice_w,
                                                        float dice_eps) {
  constexpr int ROW = K * HEAD_C + K;
  __shared__ float red[4][ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & 7;
  float wl[K][8], gw[K][8], gb[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    gb[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wl[k][j] = w[k * HEAD_C + sub * 8 + j];
      gw[k][j] = 0.f;
    }
  }
  // Everything accumulates the unscaled (softmax - onehot) / count; the loss scale multiplies the
  // finished values (da per pixel before its bf16 rounding, dW / db in the finalize), so it scales
  // the gradients exactly
  float invc;
  // EXT: cwl[k] = cw[k] / W; the Dice term's per-class constants (all 0 at dice_w == 0)
  [[maybe_unused]] float cwl[K], dA[K], dB[K];
  if constexpr (EXT) {
    const float sw = sums[1];
    invc = sw > 0.f ? 1.f / sw : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      cwl[k] = (cw != nullptr ? cw[k] : 1.f) * invc;
      const float dk = sums[2 + K + k] + sums[2 + 2 * K + k] + dice_eps;
      const float rk = dice_w / ((float)K * dk);
      dA[k] = -2.f * rk;
      dB[k] = rk * (2.f * sums[2 + k] + dice_eps) / dk;
    }
  } else {
    invc = 1.f / fmaxf(sums[1], 1.f);
  }
  const long stride = (long)gridDim.x * 32;
  for (long p0 = blockIdx.x * 32l + (threadIdx.x >> 3); p0 < M; p0 += stride * HPX) {
    uint4 vq[HPX];
    float xq[HPX][K];
    int lab[HPX];
#pragma unroll
    for (int u = 0; u < HPX; ++u) {
      const long p = p0 + u * stride;
      if (p < M) {
        vq[u] = *(const uint4*)(a + (size_t)p * apitch + sub * 8);
        lab[u] = labels[p];
#pragma unroll
        for (int k = 0; k < K; ++k) xq[u][k] = logits[(size_t)p * K + k];  // all 8 lanes: one broadcast line
      }
    }
#pragma unroll
    for (int u = 0; u < HPX; ++u) {
      const long p = p0 + u * stride;
      if (p >= M) break;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = 0.f;
      if (lab[u] < K) {  // kept pixel (the 8 lanes of the group agree)
        float mx = xq[u][0];
#pragma unroll
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, xq[u][k]);
        float e[K], se = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          e[k] = __expf(xq[u][k] - mx);
          se += e[k];
        }
        const float inv = 1.f / se;
        float f[8];
        unpack8(vq[u], f);
        [[maybe_unused]] float wt = 0.f, dot = 0.f, G[K];
        if constexpr (EXT) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            if (k == lab[u]) wt = cwl[k];
            G[k] = dB[k] + (k == lab[u] ? dA[k] : 0.f);
            dot = fmaf(G[k], e[k] * inv, dot);
          }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
          float dl;
          if constexpr (EXT) {
            // the CE part rounds as the plain kernel's contracted e * inv - onehot does: with unit weights and
            // dice_w == 0 (G = dot = 0) the two modes agree bitwise
            dl = fmaf(e[k], inv, k == lab[u] ? -1.f : 0.f) * wt + (e[k] * inv) * (G[k] - dot);
          } else {
            dl = (e[k] * inv - (k == lab[u] ? 1.f : 0.f)) * invc;
          }
          gb[k] += dl;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            gw[k][j] = fmaf(dl, f[j], gw[k][j]);
            o[j] = fmaf(dl, wl[k][j], o[j]);
          }
        }
      }
      uint4 ov;
      ov.x = pack2bf(o[0] * gscale, o[1] * gscale);
      ov.y = pack2bf(o[2] * gscale, o[3] * gscale);
      ov.z = pack2bf(o[4] * gscale, o[5] * gscale);
      ov.w = pack2bf(o[6] * gscale, o[7] * gscale);
      *(uint4*)(da + (size_t)p * dapitch + sub * 8) = ov;
    }
  }
  // reduce over the 8 pixel groups of the wave that share `sub` (gb: every lane of a group holds the
  // same value, so the same three steps leave the wave total in every lane)
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = gw[k][j];
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      gw[k][j] = v;
    }
    float g = gb[k];
    g += __shfl_xor(g, 8, 64);
    g += __shfl_xor(g, 16, 64);
    g += __shfl_xor(g, 32, 64);
    gb[k] = g;
  }
  if (lane < 8) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wave][k * HEAD_C + lane * 8 + j] = gw[k][j];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave][K * HEAD_C + k] = gb[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ROW; c += 256)
    partial[(size_t)blockIdx.x * ROW + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

// gw[0 .. K*64) = dW in [K][64] order, gbias[0 .. K) = db, both times the loss scale: one block per
// column of the [T][row] partials
__global__ void headk_grad_finalize_kernel(const float* __restrict__ partial, int T, int row, int nw, float gscale,
                                           float* __restrict__ gw, float* __restrict__ gbias) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int t = threadIdx.x; t < T; t += 256) s += partial[(size_t)t * row + c];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = (red[0] + red[1] + red[2] + red[3]) * gscale;
    if (c < nw) gw[c] = tot; else gbias[c - nw] = tot;
  }
}

template <int K>
__global__ __launch_bounds__(256) void headk_mask_kernel(const u16* __restrict__ a, int apitch,
                                                         const float* __restrict__ w, const float* __restrict__ b,
                                                         int cls, uint8_t* __restrict__ mask, int M) {
  constexpr int KP = pow2_classes(K);
  const int sub = threadIdx.x & 7;
  const int kk = sub & (KP - 1);
  const bool own = kk < K;
  float wl[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) wl[k][j] = w[k * HEAD_C + sub * 8 + j];
  const float bias = own ? b[kk] : 0.f;
  const long stride = (long)gridDim.x * 32;
  // (the trip count is the same for the 8 lanes of a group, and the shuffles stay inside the group)
  for (long p = blockIdx.x * 32l + (threadIdx.x >> 3); p < M; p += stride) {
    const uint4 v = *(const uint4*)(a + (size_t)p * apitch + sub * 8);
    float f[8];
    unpack8(v, f);
    const int idx = argmax_lowest<K>(lane_logit<K>(f, wl, sub) + bias, sub);
    if (sub == 0) mask[p] = idx == cls ? 1 : 0;
  }
}

int blocks_for(long M) { return (int)std::max<long>(1, std::min<long>((M + 31) / 32, 2048)); }

// extended mode: class weights given, or a Dice term; otherwise the plain kernels, launched as ever
bool headk_ext(const float* cw, float dice_w) { return cw != nullptr || dice_w != 0.f; }

template <int K>
void launch_fwd(int nb, hipStream_t s, const void* a, int apitch, const float* w, const float* b, const void* labels,
                float* logits, float* partial, int M, bool ext, const float* cw) {
  if (ext)
    hipLaunchKernelGGL((headk_fwd_kernel<K, true>), dim3(nb), dim3(256), 0, s, (const u16*)a, apitch, w, b,
                       (const uint8_t*)labels, logits, partial, M, cw);
  else
    hipLaunchKernelGGL((headk_fwd_kernel<K, false>), dim3(nb), dim3(256), 0, s, (const u16*)a, apitch, w, b,
                       (const uint8_t*)labels, logits, partial, M, (const float*)nullptr);
}

template <int K>
void launch_bwd(int nb, hipStream_t s, const void* a, int apitch, const float* w, const float* logits,
                const void* labels, const float* sums, void* da, int dapitch, float* partial, int M, float gscale,
                bool ext, const float* cw, float dice_w, float dice_eps) {
  if (ext)
    hipLaunchKernelGGL((headk_bwd_kernel<K, true>), dim3(nb), dim3(256), 0, s, (const u16*)a, apitch, w, logits,
                       (const uint8_t*)labels, sums, (u16*)da, dapitch, partial, M, gscale, cw, dice_w, dice_eps);
  else
    hipLaunchKernelGGL((headk_bwd_kernel<K, false>), dim3(nb), dim3(256), 0, s, (const u16*)a, apitch, w, logits,
                       (const uint8_t*)labels, sums, (u16*)da, dapitch, partial, M, gscale, (const float*)nullptr,
                       0.f, 1.f);
}

template <int K>
void launch_mask(int nb, hipStream_t s, const void* a, int apitch, const float* w, const float* b, int cls, void* mask,
                 int M) {
  hipLaunchKernelGGL(headk_mask_kernel<K>, dim3(nb), dim3(256), 0, s, (const u16*)a, apitch, w, b, cls,
                     (uint8_t*)mask, M);
}

#define HEADK_DISPATCH(K, FN, ...)          \
  switch (K) {                              \
    case 2: FN<2>(__VA_ARGS__); break;      \
    case 3: FN<3>(__VA_ARGS__); break;      \
    case 4: FN<4>(__VA_ARGS__); break;      \
    case 5: FN<5>(__VA_ARGS__); break;      \
    case 6: FN<6>(__VA_ARGS__); break;      \
    case 7: FN<7>(__VA_ARGS__); break;      \
    case 8: FN<8>(__VA_ARGS__); break;      \
    default: return -1;                     \
  }

}  // namespace

extern "C" {
int rdp_headk_partial_blocks(long M) { return blocks_for(M); }

int rdp_headk_fwd(const void* a, int apitch, const float* w, const float* b, const void* labels, float* logits,
                  float* partial, float* sums, float* loss, int M, int K, const float* cw, float dice_w,
                  float dice_eps, hipStream_t s) {
  if (apitch % 8 || M <= 0 || !(dice_w >= 0.f) || !(dice_eps > 0.f)) return -1;
  const int nb = blocks_for(M);
  const bool ext = headk_ext(cw, dice_w);
  HEADK_DISPATCH(K, launch_fwd, nb, s, a, apitch, w, b, labels, logits, partial, M, ext, cw)
  if (ext)
    hipLaunchKernelGGL(headk_loss_finalize_ext_kernel, dim3(1), dim3(256), 0, s, partial, nb, K, dice_w, dice_eps,
                       sums, loss);
  else
    hipLaunchKernelGGL(headk_loss_finalize_kernel, dim3(1), dim3(128), 0, s, partial, nb, sums, loss);
  return nb;
}

int rdp_headk_bwd(const void* a, int apitch, const float* w, const float* logits, const void* labels,
                  const float* sums, void* da, int dapitch, float* partial, float* gw, float* gb, int M, int K,
                  float gscale, const float* cw, float dice_w, float dice_eps, hipStream_t s) {
  if (apitch % 8 || dapitch % 8 || M <= 0 || !(dice_w >= 0.f) || !(dice_eps > 0.f)) return -1;
  const int nb = blocks_for(M);
  HEADK_DISPATCH(K, launch_bwd, nb, s, a, apitch, w, logits, labels, sums, da, dapitch, partial, M, gscale,
                 headk_ext(cw, dice_w), cw, dice_w, dice_eps)
  const int row = K * HEAD_C + K;
  hipLaunchKernelGGL(headk_grad_finalize_kernel, dim3(row), dim3(256), 0, s, partial, nb, row, K * HEAD_C,
                     gscale, gw, gb);
  return nb;
}

int rdp_headk_mask(const void* a, int apitch, const float* w, const float* b, int cls, void* mask, int M, int K,
                   hipStream_t s) {
  if (apitch % 8 || M <= 0 || cls < 0 || cls >= K) return -1;
  HEADK_DISPATCH(K, launch_mask, blocks_for(M), s, a, apitch, w, b, cls, mask, M)
  return 0;
}
}
