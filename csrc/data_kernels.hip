// Training-data kernels: the per-sample resizes of the reference's SegmentationDataset on the GPU.
//
// /root/reference/scripts/train_segmenter.py:84-90 loads each colour image, converts BGR -> RGB and
// resizes it with cv2.INTER_AREA to 256x256, and resizes the mask with INTER_NEAREST -- per sample,
// on the host, every epoch. Here the decoded full-size u8 images are uploaded once and resized on the
// device into a device-resident u8 dataset (3 x 256 x 256 B = 192 KiB per sample: a million samples
// fit in 288 GB of HBM), so epochs gather batches on the GPU with no host work at all.
//
// resize_area_u8: separable INTER_AREA (area-overlap weights per output row / column, precomputed on
//   the host exactly as data/image_io.py:_area_weights), fp64 accumulation, round-half-even to u8
//   (numpy rint, the oracle's rounding), optional BGR -> RGB swap; C in {1, 3, 4}.
//
// batch_augment: the fused batch gather of a training step, with per-sample augmentation. One launch
//   reads the resident u8 samples idx[0..N) and writes the executor's input (bf16 NHWC, 8 channels,
//   channels 3-7 zero) and target directly. Per sample a 2x3 inverse affine map (output pixel -> source
//   coordinates, pixel centres at integers) and a gain / bias: the image is sampled bilinearly over the
//   v/255 values (a tap outside the frame contributes 0), out = clamp(gain * c + bias, 0, 1); the mask is
//   sampled at the nearest pixel (outside the frame: 0, or label 255 for a K-class u8 target). With the
//   identity map, gain 1 and bias 0 the weights are exactly 1 / 0 and the outputs are bit for bit what
//   index_select + data/device_data.py:batch_to_float + UNetExecutor.set_input produce (the oracle:
//   data/augment.py:augment_batch_reference).
#include "common.h"
#include "rdp_api.h"

#define AREA_MAXTAP 32

__global__ __launch_bounds__(256) void resize_area_u8_kernel(const uint8_t* __restrict__ in, int h, int w, int C,
                                                             const int* __restrict__ ys, const int* __restrict__ yn,
                                                             const double* __restrict__ yw,
                                                             const int* __restrict__ xs, const int* __restrict__ xn,
                                                             const double* __restrict__ xw, int H, int W, int swap_rb,
                                                             uint8_t* __restrict__ out) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= H * W) return;
  const int oy = o / W, ox = o - oy * W;
  const int y0 = ys[oy], ny = yn[oy], x0 = xs[ox], nx = xn[ox];
  // rows first, then columns: the oracle's order (data/image_io.py:resize_area)
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < nx; ++i) {
    const double wx = xw[(size_t)ox * AREA_MAXTAP + i];
    double col[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < ny; ++j) {
      const double wy = yw[(size_t)oy * AREA_MAXTAP + j];
      const uint8_t* px = in + ((size_t)(y0 + j) * w + x0 + i) * C;
      for (int c = 0; c < C; ++c) col[c] += wy * (double)px[c];
    }
    for (int c = 0; c < C; ++c) acc[c] += wx * col[c];
  }
  uint8_t* dst = out + (size_t)o * C;
  for (int c = 0; c < C; ++c) {
    const int sc = (swap_rb && C >= 3 && c < 3) ? 2 - c : c;
    const double v = rint(acc[sc]);
    dst[c] = (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
  }
}

// fp32 -> bf16 bits, round to nearest even (finite inputs only: the values are clamped to [0, 1])
__device__ __forceinline__ unsigned bf16_rne_bits(float v) {
  const unsigned u = __float_as_uint(v);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// One output pixel per lane: one 16-byte store of the 8 bf16 channels and one target store. The sources
// are gathered (up to 4 taps x 3 bytes + 1 mask byte per pixel, L2-resident neighbours); x offsets are
// 64-bit (a resident set passes 2 GiB at ~11 k samples of 256 x 256).
__global__ __launch_bounds__(256) void batch_augment_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ y,
                                                            const int* __restrict__ idx,
                                                            const float* __restrict__ params, int S, int H, int W,
                                                            long long total, uint4* __restrict__ x_out,
                                                            float* __restrict__ tgt_f, uint8_t* __restrict__ tgt_u) {
  // v / 255 divided in fp64 and rounded to fp32: bitwise data/device_data.py:_u8_lut
  __shared__ float lut[256];
  lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
  __syncthreads();
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int hw = H * W;
  const int n = (int)(o / hw);
  const int p = (int)(o - (long long)n * hw);
  const int oy = p / W, ox = p - oy * W;
  const int s = idx[n];
  unsigned c01 = 0u, c2 = 0u;
  float tf = 0.f;
  uint8_t tu = 255;
  if (s >= 0 && s < S) {  // an index outside the resident set reads nothing: zeros / ignore labels
    const float* m = params + (size_t)n * 8;
    const float fx = (float)ox, fy = (float)oy;
    float sx = fmaf(m[0], fx, fmaf(m[1], fy, m[2]));
    float sy = fmaf(m[3], fx, fmaf(m[4], fy, m[5]));
    // every tap of a coordinate below -1 or above the last index is outside the frame: clamping there
    // changes no result and keeps the float -> int conversions in range whatever the matrix holds
    sx = fminf(fmaxf(sx, -2.f), (float)W + 1.f);
    sy = fminf(fmaxf(sy, -2.f), (float)H + 1.f);
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float ax = sx - x0f, ay = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float wgt[4] = {(1.f - ax) * (1.f - ay), ax * (1.f - ay), (1.f - ax) * ay, ax * ay};
    const uint8_t* xs = x + (size_t)s * hw * 3;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
      if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H) {
        const uint8_t* px = xs + ((size_t)yy * W + xx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(wgt[t], lut[px[c]], acc[c]);
      }
    }
    const float gain = m[6], bias = m[7];
    unsigned b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = bf16_rne_bits(fminf(fmaxf(fmaf(gain, acc[c], bias), 0.f), 1.f));
    c01 = b[0] | (b[1] << 16);
    c2 = b[2];
    const int jx = (int)floorf(sx + 0.5f), jy = (int)floorf(sy + 0.5f);
    if ((unsigned)jx < (unsigned)W && (unsigned)jy < (unsigned)H) {
      tu = y[(size_t)s * hw + (size_t)jy * W + jx];
      tf = lut[tu];
    }
  }
  x_out[o] = make_uint4(c01, c2, 0u, 0u);
  if (tgt_f) tgt_f[o] = tf;
  else tgt_u[o] = tu;
}

extern "C" {
int rdp_batch_augment(const void* x, const void* y, const int* idx, const float* params, int S, int N, int H, int W,
                      void* x_out, float* tgt_f, void* tgt_u, hipStream_t s) {
  if ((tgt_f == nullptr) == (tgt_u == nullptr)) return -1;
  if (S < 1 || N < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return -1;
  const long long total = (long long)N * H * W;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(batch_augment_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint8_t*)x,
                     (const uint8_t*)y, idx, params, S, H, W, total, (uint4*)x_out, tgt_f, (uint8_t*)tgt_u);
  return 0;
}

int rdp_area_maxtap() { return AREA_MAXTAP; }

int rdp_resize_area_u8(const void* in, int h, int w, int C, const int* ys, const int* yn, const double* yw,
                       const int* xs, const int* xn, const double* xw, int H, int W, int swap_rb, void* out,
                       hipStream_t s) {
  if (C < 1 || C > 4) return -1;
  const int n = H * W;
  hipLaunchKernelGGL(resize_area_u8_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)in, h, w, C, ys,
                     yn, yw, xs, xn, xw, H, W, swap_rb, (uint8_t*)out);
  return 0;
}
}
