// Confusion-matrix counts of a segmentation head's logits against its targets: the device pass behind
// the validation metrics (train/metrics.py: per-class IoU / Dice, mean IoU, pixel accuracy).
//
// seg_confusion: counts[t * KC + p] += 1 for every kept pixel with truth t and prediction p, and
//   counts[KC * KC] += 1 for every ignored pixel (KC = max(K, 2)). The kernel ADDS: the validation
//   batches of an epoch accumulate into one int64 buffer, zeroed and read back once by the caller.
//   K >= 2 (2 <= K <= 8): logits fp32 pixel-major [M][K] (the executor's layout), target u8 [M].
//     prediction = argmax_k, ties to the lowest class -- the rule of headk_mask_kernel, so a pixel is
//     scored by the class serving would pick; a label >= K (255 and K..254) is ignored, as in headk_fwd.
//   K == 1: logits fp32 [M], target fp32 [M] (the one-class executor's target); prediction =
//     logit > thr (strict, as head_mask_kernel; thr is a logit), truth = target > 0.5; a 2 x 2 matrix.
//   NaN logits are unspecified.
//
// Integer arithmetic only, so the counts are exact and independent of the launch order.
//
// Shape (every choice measured, profiles/seg_metrics.md): 1024 threads, at most 256 blocks (one per CU)
// striding over the pixels; a wave takes 4 groups of 64 consecutive pixels per pass, each load
// instruction covering 64 * K contiguous floats, the four groups' loads in flight together. Each wave
// counts into its own LDS row. A segmentation map gives a wave 1-2 distinct bins, where per-lane LDS
// atomics serialise 64-way on one address; so a wave first aggregates: broadcast the first remaining
// lane's bin, ballot the lanes that share it, add the popcount from one lane, retire them. After
// SEG_ROUNDS such rounds whatever is left is spread over many bins and takes per-lane atomics (a wave
// with 64 distinct bins would otherwise loop 64 times). At block end the 16 wave rows are folded and
// every non-zero bin takes ONE 64-bit integer atomicAdd: the grid is small because these same-address
// global atomics, not the loads, bounded the pass at 2048 blocks of 256 threads (3 x slower).
#include "common.h"
#include "rdp_api.h"
#include <algorithm>

#define SEG_WAVES 16   // waves per block
#define SEG_U 4        // 64-pixel groups a wave has in flight per pass
#define SEG_ROUNDS 2   // aggregation rounds before the per-lane atomics
#define SEG_BLOCK_PX (SEG_WAVES * 64 * SEG_U)  // pixels of one block and pass
#define SEG_MAX_BLOCKS 256

namespace {

constexpr int kc_of(int K) { return K < 2 ? 2 : K; }

// the bin of pixel p: t * KC + pred, KC * KC if ignored
template <int K>
RDP_DEV int pixel_bin(const float* __restrict__ logits, const void* __restrict__ target, long p, float thr) {
  if constexpr (K == 1) {
    const int pr = logits[p] > thr ? 1 : 0;
    const int t = ((const float*)target)[p] > 0.5f ? 1 : 0;
    return t * 2 + pr;
  } else {
    float x[K];
    if constexpr (K == 2) {
      const float2 v = *(const float2*)(logits + p * 2);
      x[0] = v.x; x[1] = v.y;
    } else if constexpr (K == 4 || K == 8) {
#pragma unroll
      for (int q = 0; q < K / 4; ++q) {
        const float4 v = *(const float4*)(logits + p * K + q * 4);
        x[q * 4] = v.x; x[q * 4 + 1] = v.y; x[q * 4 + 2] = v.z; x[q * 4 + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) x[k] = logits[p * K + k];
    }
    const int t = ((const uint8_t*)target)[p];
    float best = x[0];
    int idx = 0;
#pragma unroll
    for (int k = 1; k < K; ++k)
      if (x[k] > best) { best = x[k]; idx = k; }  // strict: ties stay with the lowest class
    return t < K ? t * K + idx : K * K;
  }
}

template <int K>
__global__ __launch_bounds__(SEG_WAVES * 64) void seg_confusion_kernel(const float* __restrict__ logits,
                                                                       const void* __restrict__ target,
                                                                       unsigned long long* __restrict__ counts,
                                                                       long M, float thr) {
  constexpr int KC = kc_of(K);
  constexpr int NB = KC * KC + 1;
  __shared__ unsigned rows[SEG_WAVES][NB];
  for (int c = threadIdx.x; c < SEG_WAVES * NB; c += SEG_WAVES * 64) (&rows[0][0])[c] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned* const row = rows[wave];
  const long stride = (long)gridDim.x * SEG_BLOCK_PX;
  for (long base = (long)blockIdx.x * SEG_BLOCK_PX + wave * (64 * SEG_U); base < M; base += stride) {  // wave-uniform
    int bin[SEG_U];
#pragma unroll
    for (int u = 0; u < SEG_U; ++u) {  // the SEG_U groups' loads are issued before the first count
      const long p = base + u * 64 + lane;
      bin[u] = p < M ? pixel_bin<K>(logits, target, p, thr) : -1;
    }
#pragma unroll
    for (int u = 0; u < SEG_U; ++u) {
      unsigned long long rem = __ballot(bin[u] >= 0);
      for (int r = 0; r < SEG_ROUNDS && rem; ++r) {
        const int leader = __ffsll(rem) - 1;
        const int b = __shfl(bin[u], leader, 64);
        const unsigned long long same = __ballot(bin[u] == b);  // b >= 0: only lanes still in `rem` can match
        if (lane == leader) atomicAdd(&row[b], (unsigned)__popcll(same));  // one uncontended ds_add per round
        rem &= ~same;
      }
      if ((rem >> lane) & 1) atomicAdd(&row[bin[u]], 1u);  // only lanes with a pixel (bin >= 0) are in `rem`
    }
  }
  __syncthreads();
  if (threadIdx.x < NB) {
    const int c = threadIdx.x;
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < SEG_WAVES; ++w) s += rows[w][c];
    if (s) atomicAdd(counts + c, s);
  }
}

template <int K>
void launch_confusion(int nb, hipStream_t s, const float* logits, const void* target, void* counts, long M, float thr) {
  hipLaunchKernelGGL(seg_confusion_kernel<K>, dim3(nb), dim3(SEG_WAVES * 64), 0, s, logits, target,
                     (unsigned long long*)counts, M, thr);
}

}  // namespace

extern "C" {
int rdp_seg_confusion_block_pixels() { return SEG_BLOCK_PX; }

int rdp_seg_confusion_blocks(long M) {
  return (int)std::max<long>(1, std::min<long>((M + SEG_BLOCK_PX - 1) / SEG_BLOCK_PX, SEG_MAX_BLOCKS));
}

int rdp_seg_confusion(const float* logits, const void* target, void* counts, long M, int K, float thr, int max_blocks,
                      hipStream_t s) {
  if (M <= 0) return -1;
  int nb = rdp_seg_confusion_blocks(M);
  if (max_blocks > 0) nb = std::min(nb, max_blocks);
  switch (K) {
    case 1: launch_confusion<1>(nb, s, logits, target, counts, M, thr); break;
    case 2: launch_confusion<2>(nb, s, logits, target, counts, M, thr); break;
    case 3: launch_confusion<3>(nb, s, logits, target, counts, M, thr); break;
    case 4: launch_confusion<4>(nb, s, logits, target, counts, M, thr); break;
    case 5: launch_confusion<5>(nb, s, logits, target, counts, M, thr); break;
    case 6: launch_confusion<6>(nb, s, logits, target, counts, M, thr); break;
    case 7: launch_confusion<7>(nb, s, logits, target, counts, M, thr); break;
    case 8: launch_confusion<8>(nb, s, logits, target, counts, M, thr); break;
    default: return -1;
  }
  return nb;
}
}
