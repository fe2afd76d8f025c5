// Connected-component filter of the serving mask: removes the 8-connected components of a u8 mask whose area is
// below min_area and, when asked, every survivor but the largest (ties: the component whose first pixel in
// row-major order comes first). In place; kept pixels keep their byte value. The definition is
// geometry/components.py filter_components_reference.
//
// One 1,024-thread workgroup per frame (blockIdx.x = frame), every piece of state in LDS and initialised by the
// launch that reads it: no workspace, no allocation, nothing waits on another workgroup.
//
// Cells. Under 8-connectivity the foreground pixels of a 2 x 2 cell are mutually connected, so the union-find
// runs over the ceil(H/2) x ceil(W/2) cells: at most 32,768 of them for H * W <= 65,536 (a one-row mask), one
// u32 word each = 128 KiB of LDS. A word is (parent cell << 8) | (links << 4) | pattern while merging:
//   pattern  bit 0..3 = the cell's pixels TL, TR, BL, BR (outside the image: 0)
//   links    the unions this cell performs: 4 = its left neighbour (only the first lane of a wave), 5 = the cell
//            below, 6 = below right, 7 = below left. A link that follows from its neighbours' links is left
//            out (a solid region performs one union per cell row and run, not three per cell).
//
// Steps (a workgroup barrier between them):
//   0  load: each cell's pattern from its 2 x 2 pixels
//   1  init: links from the six patterns around the cell; parent = the first cell of the cell's horizontal run
//      inside its wave (a ballot of the run breaks), so a run starts flat. Formed in registers, stored after a
//      barrier of its own
//   2  merge: the links' unions. find() walks parent words, which only ever decrease, and halves the path as it
//      goes; a union hooks the larger root under the smaller with a compare-and-swap that succeeds only while
//      that cell is still a root, and starts over otherwise.
//        Correctness under races: only a successful CAS changes a root, and it merges two trees into one with
//        one root; a halving store rewrites a non-root's parent to a cell that was its ancestor, which is in
//        the same tree for good. So every tree keeps exactly one root and never splits; a union returns only
//        when both ends share a root.
//        Termination: parents strictly decrease along a path, so find() ends; a CAS fails only because another
//        union hooked that root in the meantime, and at most (cells - 1) hooks ever succeed. No thread waits
//        for another. (A 256 x 256 serpentine, one 32 K-pixel path, is 128 flat runs and 127 unions.)
//   3  flatten: every cell's word points at its root, and (4) roots switch to ROOT | area << 4 | pattern, area 0
//   5  area: pixel counts added onto the roots (LDS atomics, aggregated per wave where lanes share a root)
//   6  keep_largest: block max of the surviving areas, then block min of (first pixel << 15 | root) over the
//      cells of the components that have it
//   7  write: zero the pixels of the components that do not stay; stats
//
// Reads are 16-byte vector loads (W and the frame base multiples of 16: the serving mask), 2-byte loads (even W
// and base) or guarded byte loads; writes are plain stores of zero. From step 2 on a thread owns quads of four
// consecutive cells and reads their words with one 16-byte LDS load.
#include "common.h"
#include "rdp_api.h"

#define MC_THREADS 1024
#define MC_MAX_CELLS 32768
#define MC_MAX_PIXELS 65536
#define MC_ROOT 0x80000000u

namespace {

RDP_DEV uint32_t mc_ld(const uint32_t* a, uint32_t i) {
  return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
RDP_DEV void mc_st(uint32_t* a, uint32_t i, uint32_t v) {
  __hip_atomic_store(a + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the root of cell i and its word; halves the path on the way
RDP_DEV uint32_t mc_find(uint32_t* a, uint32_t i, uint32_t& word) {
  uint32_t w = mc_ld(a, i);
  uint32_t p = w >> 8;
  while (p != i) {
    const uint32_t wp = mc_ld(a, p);
    const uint32_t gp = wp >> 8;
    if (gp == p) {
      word = wp;
      return p;
    }
    mc_st(a, i, (gp << 8) | (w & 255u));  // i is not a root (p != i) and never becomes one again
    i = gp;
    w = mc_ld(a, i);
    p = w >> 8;
  }
  word = w;
  return i;
}

RDP_DEV void mc_unite(uint32_t* a, uint32_t x, uint32_t y) {
  for (;;) {
    uint32_t wx, wy;
    x = mc_find(a, x, wx);
    y = mc_find(a, y, wy);
    if (x == y) return;
    if (x < y) {
      const uint32_t t = x; x = y; y = t;
      wx = wy;
    }
    // wx is x's word as a root; the swap succeeds only if x still is one
    if (atomicCAS(a + x, wx, (y << 8) | (wx & 255u)) == wx) return;
  }
}

RDP_DEV bool mc_h(uint32_t l, uint32_t r) { return (l & 0xAu) && (r & 0x5u); }  // right column meets left column
RDP_DEV bool mc_v(uint32_t t, uint32_t b) { return (t & 0xCu) && (b & 0x3u); }  // bottom row meets top row

RDP_DEV uint32_t mc_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the pattern of one cell from the low 16 bits of its top and bottom pixel pairs
RDP_DEV uint32_t mc_pat2(uint32_t t, uint32_t b) {
  return ((t & 0xFFu) ? 1u : 0u) | ((t & 0xFF00u) ? 2u : 0u) | ((b & 0xFFu) ? 4u : 0u) | ((b & 0xFF00u) ? 8u : 0u);
}
// eight cells' patterns from 16 top and 16 bottom pixels
RDP_DEV void mc_strip(uint32_t* dst, uint4 t, uint4 b) {
  uint4 lo, hi;
  lo.x = mc_pat2(t.x, b.x); lo.y = mc_pat2(t.x >> 16, b.x >> 16);
  lo.z = mc_pat2(t.y, b.y); lo.w = mc_pat2(t.y >> 16, b.y >> 16);
  hi.x = mc_pat2(t.z, b.z); hi.y = mc_pat2(t.z >> 16, b.z >> 16);
  hi.z = mc_pat2(t.w, b.w); hi.w = mc_pat2(t.w >> 16, b.w >> 16);
  *(uint4*)dst = lo;
  *(uint4*)(dst + 4) = hi;
}

// the root of a cell from its word, once every word is flat (steps 5 to 7)
RDP_DEV uint32_t mc_root(uint32_t i, uint32_t w) { return (w & MC_ROOT) ? i : (w >> 8) & 0x7FFFu; }
RDP_DEV uint32_t mc_area(uint32_t w) { return (w >> 4) & 0x1FFFFu; }

__global__ __launch_bounds__(MC_THREADS) void mask_components_kernel(uint8_t* mask, int H, int W, int CH, int CW,
                                                                     FastDiv dcw, int keep_largest, int min_area,
                                                                     int* stats) {
  __shared__ __attribute__((aligned(16))) uint32_t a[MC_MAX_CELLS];
  __shared__ uint32_t s_max, s_key, s_cnt[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t NC = (uint32_t)CH * (uint32_t)CW;
  uint8_t* const m = mask + (size_t)blockIdx.x * ((size_t)H * (size_t)W);
  const bool pairs = (W & 1) == 0 && ((uintptr_t)m & 1u) == 0;
  const bool wide = (W & 15) == 0 && ((uintptr_t)m & 15u) == 0;  // then 8 cells = 16 pixels never leave a row
  if (tid == 0) {
    s_max = 0u;
    s_key = 0xFFFFFFFFu;
    s_cnt[0] = s_cnt[1] = s_cnt[2] = s_cnt[3] = 0u;
  }

  // ---- 0: patterns. Wide form: 16-byte loads, two strips of 8 cells per thread in flight (a 256 x 256 mask is
  // four loads per thread, issued together, instead of sixteen rounds of 2-byte loads: profiles/mask_components.md)
  if (wide) {
    const uint32_t ns = NC >> 3;
    for (uint32_t s0 = tid; s0 < ns; s0 += 2u * MC_THREADS) {
      const bool h1 = s0 + MC_THREADS < ns;
      const uint32_t i0 = 8u * s0, i1 = 8u * (h1 ? s0 + MC_THREADS : s0);
      const uint32_t cy0 = fdiv(i0, dcw), cy1 = fdiv(i1, dcw);
      const uint32_t cx0 = i0 - cy0 * (uint32_t)CW, cx1 = i1 - cy1 * (uint32_t)CW;
      const uint8_t* p0 = m + (size_t)(2u * cy0) * W + 2u * cx0;
      const uint8_t* p1 = m + (size_t)(2u * cy1) * W + 2u * cx1;
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      const uint4 t0 = *(const uint4*)p0;
      const uint4 b0 = 2u * cy0 + 1u < (uint32_t)H ? *(const uint4*)(p0 + W) : z;
      const uint4 t1 = *(const uint4*)p1;
      const uint4 b1 = 2u * cy1 + 1u < (uint32_t)H ? *(const uint4*)(p1 + W) : z;
      mc_strip(a + i0, t0, b0);
      if (h1) mc_strip(a + i1, t1, b1);
    }
  } else {
    for (uint32_t i = tid; i < NC; i += MC_THREADS) {
      const uint32_t cy = fdiv(i, dcw), cx = i - cy * (uint32_t)CW;
      const uint32_t y = 2u * cy, x = 2u * cx;
      const bool row1 = y + 1u < (uint32_t)H;
      uint32_t pat;
      if (pairs) {
        const uint32_t t = *(const uint16_t*)(m + (size_t)y * W + x);
        const uint32_t b = row1 ? *(const uint16_t*)(m + (size_t)(y + 1u) * W + x) : 0u;
        pat = mc_pat2(t, b);
      } else {
        const bool col1 = x + 1u < (uint32_t)W;
        const uint8_t* p = m + (size_t)y * W + x;
        pat = p[0] ? 1u : 0u;
        if (col1 && p[1]) pat |= 2u;
        if (row1 && p[W]) pat |= 4u;
        if (row1 && col1 && p[W + 1]) pat |= 8u;
      }
      a[i] = pat;
    }
  }
  __syncthreads();

  // ---- 1: links and run starts, in two halves with a barrier between them: every cell's new word is formed in
  // registers from the six patterns around it, then stored, so no word is read while it is rewritten. (This step
  // is the longest, 10 of 28 us on a realistic mask; a single pass with atomic loads beside the stores measured
  // the same: profiles/mask_components.md)
  uint32_t held[MC_MAX_CELLS / MC_THREADS];
#pragma unroll
  for (uint32_t k = 0; k < MC_MAX_CELLS / MC_THREADS; ++k) {
    if (k * MC_THREADS >= NC) break;  // uniform
    const uint32_t i = k * MC_THREADS + tid;
    const bool act = i < NC;
    uint32_t word = 0u;
    bool left = false;
    if (act) {
      const uint32_t cy = fdiv(i, dcw), cx = i - cy * (uint32_t)CW;
      const bool hl = cx > 0u, hr = cx + 1u < (uint32_t)CW, hd = cy + 1u < (uint32_t)CH;
      const uint32_t d = i + (uint32_t)CW;
      // a neighbour that does not exist reads cell i instead and is masked
      const uint32_t B = a[i] & 15u;
      const uint32_t A = a[hl ? i - 1u : i] & (hl ? 15u : 0u);
      const uint32_t C = a[hr ? i + 1u : i] & (hr ? 15u : 0u);
      const uint32_t E = a[hd ? d : i] & (hd ? 15u : 0u);
      const uint32_t D = a[hd && hl ? d - 1u : i] & (hd && hl ? 15u : 0u);
      const uint32_t F = a[hd && hr ? d + 1u : i] & (hd && hr ? 15u : 0u);
      left = mc_h(A, B);
      const bool right = mc_h(B, C), left_d = mc_h(D, E), left_f = mc_h(E, F);
      const bool down = mc_v(B, E), down_l = mc_v(A, D), down_r = mc_v(C, F);
      const bool dr = (B & 8u) && (F & 1u), dl = (B & 4u) && (D & 2u);
      word = B;
      if (left && lane == 0u) word |= 16u;
      if (down && !(left && left_d && down_l)) word |= 32u;
      if (dr && !((down && left_f) || (down_r && right))) word |= 64u;
      if (dl && !((down && left_d) || (down_l && left))) word |= 128u;
    }
    // the run of this cell inside the wave starts at the last break at or before its lane (lane 0 always breaks)
    const unsigned long long brk = __ballot(!act || !left || lane == 0u);
    const unsigned long long upto = brk & ((2ull << lane) - 1ull);
    const uint32_t s = 63u - (uint32_t)__clzll((long long)upto);
    held[k] = ((i - (lane - s)) << 8) | word;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < MC_MAX_CELLS / MC_THREADS; ++k) {
    if (k * MC_THREADS >= NC) break;
    const uint32_t i = k * MC_THREADS + tid;
    if (i < NC) a[i] = held[k];
  }
  __syncthreads();

  // From here a thread owns quads of four consecutive cells and reads their words with one 16-byte LDS load.
  // (The words beyond NC in a last, partial quad are never used.)

  // ---- 2: merge (only the link bits of the own words are used: they do not change)
  for (uint32_t q = tid; 4u * q < NC; q += MC_THREADS) {
    const uint4 v = *(const uint4*)(a + 4u * q);
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t i = 4u * q + u, w = w4[u];
      if (i >= NC || !(w & 0xF0u)) continue;
      if (w & 16u) mc_unite(a, i - 1u, i);
      if (w & 32u) mc_unite(a, i, i + (uint32_t)CW);
      if (w & 64u) mc_unite(a, i, i + (uint32_t)CW + 1u);
      if (w & 128u) mc_unite(a, i, i + (uint32_t)CW - 1u);
    }
  }
  __syncthreads();

  // ---- 3 + 4: flatten, and roots switch to ROOT | area << 4 | pattern with area 0. Only its owner writes a
  // word here; a reader that meets a root's new word sees ROOT, its old word points at itself: a root either way
  for (uint32_t q = tid; 4u * q < NC; q += MC_THREADS) {
    const uint4 v = *(const uint4*)(a + 4u * q);
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    uint32_t hop[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {  // the four first hops in flight together
      const uint32_t i = 4u * q + u;
      hop[u] = mc_ld(a, i < NC ? w4[u] >> 8 : 0u);  // unconditional (a root reads itself): one wait for the four
    }
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t i = 4u * q + u, w = w4[u], p = w >> 8;
      if (i >= NC) continue;
      if (p == i) {
        mc_st(a, i, MC_ROOT | (w & 15u));
        continue;
      }
      uint32_t r = p, wr = hop[u];
      while (!(wr & MC_ROOT) && (wr >> 8) != r) {
        r = wr >> 8;
        wr = mc_ld(a, r);
      }
      if (r != p) mc_st(a, i, (r << 8) | (w & 255u));
    }
  }
  __syncthreads();

  // ---- 5: areas (area << 4 stays below bit 21: an add never reaches the other fields, which is all that the
  // plain reads of the own words use while the adds land)
  for (uint32_t qb = 0; 4u * qb < NC; qb += MC_THREADS) {
    const uint32_t q = qb + tid;
    const bool qact = 4u * q < NC;
    const uint4 v = qact ? *(const uint4*)(a + 4u * q) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t i = 4u * q + u, w = w4[u];
      const uint32_t cnt = (qact && i < NC) ? (uint32_t)__popc(w & 15u) : 0u;
      const uint32_t root = mc_root(i, w);
      const bool has = cnt > 0u;
      unsigned long long rem = __ballot(has);
      if (!rem) continue;  // wave-uniform
      const unsigned long long b0 = __ballot(cnt & 1u), b1 = __ballot(cnt & 2u), b2 = __ballot(cnt & 4u);
      for (int r = 0; r < 2 && rem; ++r) {  // lanes that share the first remaining lane's root add once
        const int leader = __ffsll((long long)rem) - 1;
        const uint32_t b = (uint32_t)__shfl((int)root, leader, 64);
        const unsigned long long same = __ballot(has && root == b) & rem;
        if ((int)lane == leader) {
          const uint32_t s = (uint32_t)__popcll(same & b0) + 2u * (uint32_t)__popcll(same & b1) +
                             4u * (uint32_t)__popcll(same & b2);
          atomicAdd(a + b, s << 4);
        }
        rem &= ~same;
      }
      if ((rem >> lane) & 1ull) atomicAdd(a + root, cnt << 4);
    }
  }
  __syncthreads();

  // ---- 6: the largest survivor, ties to the first pixel
  uint32_t winner = 0xFFFFFFFFu;
  if (keep_largest) {
    uint32_t mx = 0u;
    for (uint32_t q = tid; 4u * q < NC; q += MC_THREADS) {
      const uint4 v = *(const uint4*)(a + 4u * q);
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t u = 0; u < 4u; ++u)
        if (4u * q + u < NC && (w4[u] & MC_ROOT) && mc_area(w4[u]) >= (uint32_t)min_area) mx = max(mx, mc_area(w4[u]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    if (lane == 0u && mx) atomicMax(&s_max, mx);
    __syncthreads();
    const uint32_t best = s_max;
    uint32_t key = 0xFFFFFFFFu;
    if (best) {
      for (uint32_t q = tid; 4u * q < NC; q += MC_THREADS) {
        const uint4 v = *(const uint4*)(a + 4u * q);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t ar[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
          const uint32_t i = 4u * q + u;
          const bool fg = i < NC && (w4[u] & 15u);
          ar[u] = mc_area(a[fg ? mc_root(i, w4[u]) : 0u]) & (fg ? 0x1FFFFu : 0u);  // unconditional loads: one wait
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
          if (ar[u] != best) continue;  // best > 0: a cell without foreground never matches
          const uint32_t i = 4u * q + u, pat = w4[u] & 15u;
          const uint32_t cy = fdiv(i, dcw), cx = i - cy * (uint32_t)CW;
          const uint32_t f = (uint32_t)__ffs((int)pat) - 1u;  // TL < TR < BL < BR is the row-major order too
          const uint32_t pix = (2u * cy + (f >> 1)) * (uint32_t)W + 2u * cx + (f & 1u);
          key = min(key, (pix << 15) | mc_root(i, w4[u]));
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
    if (lane == 0u && key != 0xFFFFFFFFu) atomicMin(&s_key, key);
    __syncthreads();
    if (s_key != 0xFFFFFFFFu) winner = s_key & 0x7FFFu;
  }

  // ---- 7: write and count
  uint32_t c_found = 0u, c_kept = 0u, p_kept = 0u, p_removed = 0u;
  for (uint32_t q = tid; 4u * q < NC; q += MC_THREADS) {
    const uint4 v = *(const uint4*)(a + 4u * q);
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    uint32_t ar[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t i = 4u * q + u;
      const bool fg = i < NC && (w4[u] & 15u);
      ar[u] = mc_area(a[fg ? mc_root(i, w4[u]) : 0u]) & (fg ? 0x1FFFFu : 0u);
    }
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) {
      const uint32_t area = ar[u];
      if (!area) continue;  // no foreground in this cell
      const uint32_t i = 4u * q + u, root = mc_root(i, w4[u]);
      const bool kept = keep_largest ? root == winner : area >= (uint32_t)min_area;
      if (root == i) {
        ++c_found;
        if (kept) {
          ++c_kept;
          p_kept += area;
        } else {
          p_removed += area;
        }
      }
      if (kept) continue;
      const uint32_t cy = fdiv(i, dcw), cx = i - cy * (uint32_t)CW;
      const uint32_t y = 2u * cy, x = 2u * cx;
      const bool row1 = y + 1u < (uint32_t)H;
      uint8_t* p = m + (size_t)y * W + x;
      if (pairs) {
        *(uint16_t*)p = 0;
        if (row1) *(uint16_t*)(p + W) = 0;
      } else {
        const bool col1 = x + 1u < (uint32_t)W;
        p[0] = 0;
        if (col1) p[1] = 0;
        if (row1) p[W] = 0;
        if (row1 && col1) p[W + 1] = 0;
      }
    }
  }
  if (stats == nullptr) return;
  c_found = mc_wave_sum(c_found);
  c_kept = mc_wave_sum(c_kept);
  p_kept = mc_wave_sum(p_kept);
  p_removed = mc_wave_sum(p_removed);
  if (lane == 0u) {
    if (c_found) atomicAdd(&s_cnt[0], c_found);
    if (c_kept) atomicAdd(&s_cnt[1], c_kept);
    if (p_kept) atomicAdd(&s_cnt[2], p_kept);
    if (p_removed) atomicAdd(&s_cnt[3], p_removed);
  }
  __syncthreads();
  if (tid < 4u) stats[(size_t)blockIdx.x * 4 + tid] = (int)s_cnt[tid];
}

}  // namespace

extern "C" int rdp_mask_components(void* mask, int n, int H, int W, int keep_largest, int min_area, int* stats,
                                   hipStream_t s) {
  if (mask == nullptr || n < 1 || H < 1 || W < 1 || min_area < 0) return -1;
  if ((long)H * (long)W > MC_MAX_PIXELS) return -1;
  const int CH = (H + 1) / 2, CW = (W + 1) / 2;
  if ((long)CH * CW > MC_MAX_CELLS) return -1;
  hipLaunchKernelGGL(mask_components_kernel, dim3(n), dim3(MC_THREADS), 0, s, (uint8_t*)mask, H, W, CH, CW,
                     make_fastdiv((uint32_t)CW), keep_largest ? 1 : 0, min_area, stats);
  return 0;
}
