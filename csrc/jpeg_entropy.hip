// Huffman entropy decode of a marker-less baseline JPEG scan on the GPU (gfx950): the last host-serial
// stage of the colour path. jpeg_sync.h has the algorithm and the per-lane code; this file is the five
// launches around it. One lane owns one subsequence of S bits, kLanes subsequences per workgroup, the
// Huffman tables and the lanes' end states in LDS.
//
// Every grid is sized from the scan buffer's *capacity*, so one captured graph serves every frame; the
// frame's bit count is read from device memory and lanes past ceil(nbits / S) exit.
//
//   1. jpeg_zero_kernel     zero the frame's coefficient planes (16-byte stores); status word = 0
//   2. jpeg_sync_kernel     per workgroup: speculate from (t * S, 0, 0), then Jacobi rounds (each lane
//                           restarts from its left neighbour's end state) until no end state changes --
//                           at most (subsequences in the workgroup - 1) rounds, by which the whole
//                           workgroup is a chain from its first lane's start
//   3. jpeg_stitch_kernel   one workgroup walks the workgroup boundaries in order: workgroup g's first
//                           lane restarts from g - 1's (now final) end state and the rounds run again, at
//                           most (subsequences in g) of them; then the exclusive prefix sum of the blocks
//                           completed per subsequence (each lane's first block ordinal) and the statistics
//   4. jpeg_write_kernel    each lane re-decodes its subsequence from its final start and stores the AC
//                           values and DC differences; an error sets the status word
//   5. jpeg_dc_kernel       per component, the inclusive prefix sum of the DC differences in scan order
//
// No loop's trip count depends on how fast the data synchronises beyond those bounds; every store is
// guarded by the block count of the frame and of the output buffer.
#include "common.h"
#include "rdp_api.h"
#include "jpeg_sync.h"

using namespace jsync;

namespace {

struct Args {
  const uint32_t* scan;
  const int* nbits;  // device: the frame's bit count (<= cap_bits)
  const uint4* tables;
  const int* geo;
  int16_t* coefs;
  int* work;
  int* status;
  uint32_t cap_bits;
  uint32_t S;
  long cap_blocks;
  Work lay;
};

RDP_DEV uint32_t frame_bits(const Args& a) {
  const int nb = *a.nbits;
  return nb < 0 ? 0u : ((uint32_t)nb > a.cap_bits ? a.cap_bits : (uint32_t)nb);
}

RDP_DEV void stage_tables(const Args& a, Tables& T) {
  uint4* dst = reinterpret_cast<uint4*>(&T);
  for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 16); i += blockDim.x) dst[i] = a.tables[i];
  __syncthreads();
}

RDP_DEV St load_st(const int* p, long t) {
  const uint2 v = *reinterpret_cast<const uint2*>(p + 2 * t);
  return St{v.x, v.y};
}
RDP_DEV void store_st(int* p, long t, St s) { *reinterpret_cast<uint2*>(p + 2 * t) = make_uint2(s.p, s.bk); }

// The Jacobi rounds of workgroup g (lane i owns subsequence g * kLanes + i). left: the end state lane 0
// restarts from (stitch) -- without it lane 0 keeps its start. Returns the rounds run (the one that finds
// no end state changed included). in / out / cnt: this lane's start state, end state and block count, updated.
RDP_DEV int sync_rounds(const Args& a, const Tables& T, St* E, uint32_t nbits, uint32_t n, long g, bool stitch, St left,
                        St& in, St& out, int& cnt) {
  const int i = threadIdx.x;
  const long t0 = g * kLanes;
  const int nl = (int)(n - t0 < kLanes ? n - t0 : kLanes);  // workgroup-uniform
  const bool active = i < nl;
  const uint32_t t = (uint32_t)(t0 + i);
  E[i] = out;
  __syncthreads();
  int rounds = 0;
  const int bound = stitch ? nl : nl - 1;
  for (int r = 1; r <= bound; ++r) {
    St prev = in;
    if (active) prev = i > 0 ? E[i - 1] : (stitch ? left : in);
    __syncthreads();
    int ch = 0;
    if (active && !same(prev, in)) {
      in = prev;
      St o = in;
      cnt = run_spec(T, a.scan, nbits, o, sub_end(t, n, a.S, nbits));
      ch = !same(o, out);
      out = o;
      E[i] = out;
    }
    ++rounds;
    if (!__syncthreads_or(ch)) break;
  }
  return rounds;
}

__global__ __launch_bounds__(256) void jpeg_zero_kernel(const Args a) {
  const long total = a.geo[5];
  const long live = total < 0 ? 0 : (total < a.cap_blocks ? total : a.cap_blocks);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // 16 bytes each, 8 per block
  if (i == 0) *a.status = 0;
  if (i < live * 8) reinterpret_cast<uint4*>(a.coefs)[i] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kLanes) void jpeg_sync_kernel(const Args a) {
  __shared__ Tables T;
  __shared__ St E[kLanes];
  const uint32_t nbits = frame_bits(a);
  const uint32_t n = sub_count(nbits, a.S);
  const long g = blockIdx.x;
  if (g * kLanes >= (long)n) return;  // the whole workgroup
  stage_tables(a, T);
  const uint32_t t = (uint32_t)(g * kLanes + threadIdx.x);
  St in{t * a.S, 0}, out = in;
  int cnt = 0;
  if (t < n) cnt = run_spec(T, a.scan, nbits, out, sub_end(t, n, a.S, nbits));
  const int rounds = sync_rounds(a, T, E, nbits, n, g, false, in, in, out, cnt);
  if (t < n) {
    store_st(a.work + a.lay.in, t, in);
    store_st(a.work + a.lay.end, t, out);
    a.work[a.lay.cnt + t] = cnt;
  }
  if (threadIdx.x == 0) a.work[a.lay.wgr + g] = rounds;
}

__global__ __launch_bounds__(kLanes) void jpeg_stitch_kernel(const Args a) {
  __shared__ Tables T;
  __shared__ St E[kLanes];
  __shared__ int wsum[kLanes / 64];
  __shared__ St leftS;  // the end state of the workgroup before the boundary
  const uint32_t nbits = frame_bits(a);
  const uint32_t n = sub_count(nbits, a.S);
  const long nwg = ((long)n + kLanes - 1) / kLanes;  // <= a.lay.nwg: n comes from nbits <= cap_bits
  if (threadIdx.x == 0 && nwg > 1) leftS = load_st(a.work + a.lay.end, kLanes - 1);
  stage_tables(a, T);
  int rounds = 0;
  for (long g = 0; g < nwg; ++g) rounds = max(rounds, a.work[a.lay.wgr + g]);
  for (long g = 1; g < nwg; ++g) {
    const long t = g * kLanes + threadIdx.x;
    St in{0, 0}, out{0, 0};
    int cnt = 0;
    if (t < (long)n) {
      in = load_st(a.work + a.lay.in, t);
      out = load_st(a.work + a.lay.end, t);
      cnt = a.work[a.lay.cnt + t];
    }
    const St left = leftS;  // every lane reads it before sync_rounds' first barrier
    rounds += sync_rounds(a, T, E, nbits, n, g, true, left, in, out, cnt);
    if (t < (long)n) {
      store_st(a.work + a.lay.in, t, in);
      store_st(a.work + a.lay.end, t, out);
      a.work[a.lay.cnt + t] = cnt;
    }
    if (threadIdx.x == kLanes - 1) leftS = out;  // final now; only a full workgroup has a successor
    __syncthreads();
  }
  // first block ordinal of every subsequence: exclusive prefix sum of the block counts, kLanes at a time
  // (wave scan + per-wave sums in LDS, the idiom of geometry.hip block_scan_excl)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (long c0 = 0; c0 < (long)n; c0 += kLanes) {
    const long t = c0 + threadIdx.x;
    const int v = t < (long)n ? a.work[a.lay.cnt + t] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < kLanes / 64; ++k) {
      before += k < wave ? wsum[k] : 0;
      total += wsum[k];
    }
    __syncthreads();
    if (t < (long)n) a.work[a.lay.ord + t] = carry + before + x - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.work[a.lay.stats] = (int)n;
    a.work[a.lay.stats + 1] = rounds;
  }
}

__global__ __launch_bounds__(kLanes) void jpeg_write_kernel(const Args a) {
  __shared__ Tables T;
  const uint32_t nbits = frame_bits(a);
  const uint32_t n = sub_count(nbits, a.S);
  if ((long)blockIdx.x * kLanes >= (long)n) return;
  stage_tables(a, T);
  const long t = (long)blockIdx.x * kLanes + threadIdx.x;
  if (t >= (long)n) return;
  const Geo G = make_geo(a.geo, T.nb, a.cap_blocks);
  const St in = load_st(a.work + a.lay.in, t);
  const long ord = a.work[a.lay.ord + t];
  if (run_write(T, G, a.scan, nbits, in, sub_end((uint32_t)t, n, a.S, nbits), t == (long)n - 1, ord, a.coefs))
    *a.status = 1;
}

// one workgroup per component; kLanes blocks per pass with a running carry
__global__ __launch_bounds__(kLanes) void jpeg_dc_kernel(const Args a) {
  __shared__ uint32_t wsum[kLanes / 64];
  const int c = blockIdx.x;
  if (c >= a.geo[2]) return;
  const Geo G = make_geo(a.geo, 1, a.cap_blocks);
  if (G.h[c] < 1 || G.v[c] < 1) return;
  const long live = G.total < G.cap ? G.total : G.cap;
  const long nblk = (long)G.bw[c] * a.geo[11 + 8 * c];
  const long bound = nblk < a.cap_blocks ? nblk : a.cap_blocks;  // from the buffer size
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (long c0 = 0; c0 < bound; c0 += kLanes) {
    const long j = c0 + threadIdx.x;
    long blk = -1;
    if (j < nblk) blk = dc_block_index(G, c, j);
    const bool ok = blk >= 0 && blk < live;
    uint32_t x = ok ? (uint32_t)(int32_t)a.coefs[blk * 64] : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < kLanes / 64; ++k) {
      before += k < wave ? wsum[k] : 0u;
      total += wsum[k];
    }
    __syncthreads();
    if (ok) a.coefs[blk * 64] = (int16_t)(carry + before + x);
    carry += total;
  }
}

}  // namespace

extern "C" int rdp_jpeg_entropy_gpu(const void* scan, long cap_bytes, const int* nbits, const void* tables,
                                    const int* geo, void* coefs, long cap_coefs, int* work, long work_words,
                                    int* status, int S, long* stats_word, hipStream_t st) {
  if (S == 0) S = kDefaultBits;
  if (S < 64 || S % 32 || cap_bytes <= 0 || cap_bytes % 4 || cap_bytes >= (1L << 28) || cap_coefs < 64) return -1;
  if (((uintptr_t)scan & 3) || ((uintptr_t)tables & 15) || ((uintptr_t)coefs & 15) || ((uintptr_t)work & 7)) return -1;
  Args a;
  a.scan = (const uint32_t*)scan;
  a.nbits = nbits;
  a.tables = (const uint4*)tables;
  a.geo = geo;
  a.coefs = (int16_t*)coefs;
  a.work = work;
  a.status = status;
  a.cap_bits = (uint32_t)(cap_bytes * 8);
  a.S = (uint32_t)S;
  a.cap_blocks = cap_coefs / 64;
  a.lay = work_layout(cap_bytes, S);
  if (work_words < a.lay.words) return -1;
  if (stats_word) *stats_word = a.lay.stats;
  const unsigned zero_grid = (unsigned)((a.cap_blocks * 8 + 255) / 256);
  hipLaunchKernelGGL(jpeg_zero_kernel, dim3(zero_grid), dim3(256), 0, st, a);
  hipLaunchKernelGGL(jpeg_sync_kernel, dim3((unsigned)a.lay.nwg), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(jpeg_stitch_kernel, dim3(1), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)a.lay.nwg), dim3(kLanes), 0, st, a);
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3), dim3(kLanes), 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
