// BatchNorm coefficient layout and the per-channel BN arithmetic of the training passes, each piece
// once. norm_act.hip, pool_up.hip, head_loss.hip and the conv epilogues that fuse a BN pass all
// compile these definitions, so "as bn_relu_apply would store it" / "as the standalone reduce would"
// hold by construction. Not so in three fused kernels of pool_up.hip (bn_relu_apply_pool, maxpool2_bwd_bn_reduce,
// upsample2_bwd<BNR>) and one line of head_bn_bwd_apply: the shared forms measured slower there, so they keep
// hand-written copies of this arithmetic (marked in place) that must change with it. The block fold of the
// (sg, sgx) sums into a partial row is not here for the same reason: its three users each keep their own.
#pragma once

// ---- layout (plain C++: also read by bindings.cpp) ----
// coef  = bn_finalize's block  [mean | invstd | scale | shift], scale = gamma * invstd,
//         shift = beta - mean * scale;  BN_ROWS * C floats.
// coef2 = bn_bwd_finalize's block [A | B | K]: dy = A * g + B * y + K;  BN2_ROWS * C floats.
enum { BN_MEAN = 0, BN_INVSTD = 1, BN_SCALE = 2, BN_SHIFT = 3, BN_ROWS = 4 };
enum { BN2_A = 0, BN2_B = 1, BN2_K = 2, BN2_ROWS = 3 };
// offset of row `row` in a C-channel coefficient block (either kind)
constexpr int bn_off(int row, int C) { return row * C; }

#ifdef __HIPCC__
#include "vec_dev.h"

// 8 consecutive channels c .. c + 7 of one row
RDP_DEV void bn_ld8(const float* block, int row, int C, int c, float* f) { ld8(block + bn_off(row, C) + c, f); }
// 4 consecutive channels c .. c + 3 of one row (the conv epilogues' MFMA fragment quads)
RDP_DEV void bn_ld4(const float* block, int row, int C, int c, float* f) {
  const float4 a = *(const float4*)(block + bn_off(row, C) + c);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
}

// ---- one channel ----
// forward: relu(y * scale + shift) in fp32; relu = 0 leaves the affine value
RDP_DEV float bn_relu(float y, float sc, float sh, int relu = 1) {
  const float z = fmaf(y, sc, sh);
  return relu ? fmaxf(z, 0.f) : z;
}
// ... rounded to bf16: the activation exactly as bn_relu_apply stores it
RDP_DEV float bn_relu_bf(float y, float sc, float sh) { return bfround(bn_relu(y, sc, sh)); }
// backward: the gradient behind the ReLU, g = da where y * scale + shift > 0, else 0
RDP_DEV float bn_relu_grad(float da, float y, float sc, float sh, int relu = 1) {
  return (!relu || fmaf(y, sc, sh) > 0.f) ? da : 0.f;
}
// backward reduce: sg += g, sgx += g * xhat, xhat = (y - mean) * invstd
RDP_DEV void bn_acc(float g, float y, float mean, float inv, float& sg, float& sgx) {
  sg += g;
  sgx += g * (y - mean) * inv;
}
// backward apply: dy = A * g + B * y + K
RDP_DEV float bn_bwd_apply(float g, float y, float A, float B, float K) { return fmaf(A, g, fmaf(B, y, K)); }

// forward statistics of 4 outputs as stored (bf16): s1 += q, s2 += q * q
RDP_DEV void bn_stats4(const uint2& v, float (&s1)[4], float (&s2)[4]) {
  const float q0 = bflo(v.x), q1 = bfhi(v.x), q2 = bflo(v.y), q3 = bfhi(v.y);
  s1[0] += q0; s2[0] += q0 * q0;
  s1[1] += q1; s2[1] += q1 * q1;
  s1[2] += q2; s2[2] += q2 * q2;
  s1[3] += q3; s2[3] += q3 * q3;
}

// ---- N channels per thread (8 in the passes, 4 in the conv epilogues) ----
template <int N>
RDP_DEV void bn_relu_n(float (&f)[N], const float (&sc)[N], const float (&sh)[N], int relu = 1) {
#pragma unroll
  for (int k = 0; k < N; ++k) f[k] = bn_relu(f[k], sc[k], sh[k], relu);
}
template <int N>
RDP_DEV void bn_relu_bf_n(float (&f)[N], const float (&sc)[N], const float (&sh)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) f[k] = bn_relu_bf(f[k], sc[k], sh[k]);
}
// masked gradient of da (ReLU on y) accumulated into (sg, sgx)
template <int N>
RDP_DEV void bn_acc_n(const float (&da)[N], const float (&y)[N], const float (&mean)[N], const float (&inv)[N],
                      const float (&sc)[N], const float (&sh)[N], float (&sg)[N], float (&sgx)[N],
                      int relu = 1) {
#pragma unroll
  for (int k = 0; k < N; ++k) bn_acc(bn_relu_grad(da[k], y[k], sc[k], sh[k], relu), y[k], mean[k], inv[k], sg[k], sgx[k]);
}
#endif  // __HIPCC__
