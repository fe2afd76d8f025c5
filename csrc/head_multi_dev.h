// Device code of the K-class 1x1 head (64 -> K, 2 <= K <= 8) that more than one kernel must run
// IDENTICALLY: the per-pixel logits and the arg-max of head_multi.hip's kernels, and the row-ring conv's
// fused K-class serving head (conv_ring.hip, HK variant). The fused head's mask has to equal
// headk_mask_kernel's bit for bit -- an arg-max over logits summed in another order flips pixels at
// near-ties -- so both include this header and compile the same fmaf chain, the same addition tree and
// the same tie rule for every K. Change nothing here without both in mind.
//
// The ring kernel has no registers for all K x 8 weights of a lane at once, so it calls class_dot per class (weights
// from LDS) and then reduce_transpose / argmax_lowest: the very pieces lane_logit is made of.
//
// Layout both callers use: 8 lanes per pixel, lane `sub` (= lane & 7) holds the pixel's channels
// 8 sub .. 8 sub + 7 (one 16-B read of 8 bf16) and the head weights wl[k][j] = w[k][8 sub + j].
#pragma once
#include "vec_dev.h"

namespace rdp_headk {

constexpr int pow2_classes(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : 8; }

// v[k] = this lane's partial of logit k (0 for the padding k >= K). Returns the full sum over the
// pixel's 8 lanes of logit (sub & (KP - 1)).
template <int KP>
RDP_DEV float reduce_transpose(float (&v)[KP], int sub) {
#pragma unroll
  for (int h = KP / 2; h >= 1; h >>= 1) {
    const bool up = (sub & h) != 0;
#pragma unroll
    for (int j = 0; j < h; ++j) {
      // (both values read first: a select between the two ADDRESSES is a dynamic index, which keeps the
      // whole array out of registers; the sums are the same either way)
      const float lo = v[j], hi = v[j + h];
      const float send = up ? lo : hi;
      const float keep = up ? hi : lo;
      v[j] = keep + __shfl_xor(send, h, 64);
    }
  }
  float r = v[0];
#pragma unroll
  for (int o = KP; o < 8; o <<= 1) r += __shfl_xor(r, o, 64);
  return r;
}

// this lane's partial of one class's logit: its 8 channels `f` against that class's 8 weights `w`
RDP_DEV float class_dot(const float* f, const float* w) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s = fmaf(f[j], w[j], s);
  return s;
}

// the logit this lane owns for the pixel whose 8 channels it holds in `f` (bias not added)
template <int K>
RDP_DEV float lane_logit(const float* f, const float (&wl)[K][8], int sub) {
  constexpr int KP = pow2_classes(K);
  float d[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) d[k] = k < K ? class_dot(f, wl[k < K ? k : 0]) : 0.f;
  return reduce_transpose<KP>(d, sub);
}

// The pixel's arg-max class, ties to the lowest, from the logit this lane owns: x = lane_logit + b[sub & (KP - 1)]
// (any value for a lane that owns a padding class). Every lane of the pixel's group returns the same class.
template <int K>
RDP_DEV int argmax_lowest(float x, int sub) {
  constexpr int KP = pow2_classes(K);
  const int kk = sub & (KP - 1);
  if (kk >= K) x = -INFINITY;
  int idx = kk;
#pragma unroll
  for (int o = 1; o < KP; o <<= 1) {
    const float ox = __shfl_xor(x, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ox > x || (ox == x && oi < idx)) { x = ox; idx = oi; }
  }
  return idx;
}

}  // namespace rdp_headk
