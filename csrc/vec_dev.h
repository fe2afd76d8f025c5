// Packed-bf16 vector helpers shared by every kernel that streams NHWC bf16: a uint32 holds two
// channels (low half = even channel), a uint2 four, a uint4 eight. One definition each, so passes
// that must agree bit for bit (norm_act / pool_up / head_loss / the conv epilogues) unpack, round
// and pack the same way.
#pragma once
#include "common.h"

RDP_DEV float bflo(uint32_t w) { return __uint_as_float(w << 16); }          // even channel of a pair
RDP_DEV float bfhi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }  // odd channel of a pair
RDP_DEV float bfround(float f) { return bf2f(f2bf(f)); }                     // f as a bf16 store would keep it

RDP_DEV void unpack4(const uint2& v, float* f) {
  f[0] = bflo(v.x); f[1] = bfhi(v.x); f[2] = bflo(v.y); f[3] = bfhi(v.y);
}
RDP_DEV void unpack8(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = bflo(w[k]);
    f[2 * k + 1] = bfhi(w[k]);
  }
}
RDP_DEV uint4 pack8(const float* f) {
  uint4 v;
  v.x = pack2bf(f[0], f[1]);
  v.y = pack2bf(f[2], f[3]);
  v.z = pack2bf(f[4], f[5]);
  v.w = pack2bf(f[6], f[7]);
  return v;
}
// 8 consecutive floats (16-B aligned) as two 16-B loads
RDP_DEV void ld8(const float* p, float* f) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
