// Convolution weight gradient, NHWC bf16 in, fp32 out; MFMA 16x16x32 over pixels.
//
// Replaces the cuDNN/MIOpen wgrad that autograd launches for every nn.Conv2d of the reference
// U-Net (/root/reference/scripts/train_segmenter.py:162 loss.backward()).
//
// GEMM view: dW^T[col = (tap, cin)][cout] = sum_pixels im2col(x)[pix][col] * dY[pix][cout].
// The reduction (pixel) axis is the strided one in NHWC, so both operand tiles are staged as
// natural [64 pixels][64 channels] rows by LDS-DMA (zero halo via out-of-range offsets) and read
// as MFMA fragments with ds_read_b64_tr_b16 (hardware transpose). The 16-B chunk of each LDS row
// is XOR-swizzled on the SOURCE address (LDS-DMA writes lane-linear) with a swizzle that makes the
// transposed reads bank-conflict free (derived by simulation; see tests/test_lds_swizzle.py).
//
// Block = 4 waves; wave w owns col-subtile w (64 (tap,cin) columns) x 64 output channels.
// Split-K over pixels; each split writes an fp32 slab [split][Cout][ncols_pad]; rdp_wgrad_reduce
// sums the splits into the parameter-gradient layout (OHWI, i.e. channels_last OIHW).
//
// Measured dead ends (kept out of the code, numbers from scripts/conv_microbench.py at bs32):
//   * STAGES=3 (one block/CU) and BKP=32 variants: slower than (64, 2) on every layer.
//   * software L2 prefetch with 4-B-per-lane loads one line per lane: 1.7x SLOWER (64 distinct
//     lines per wave-instruction saturate the address path, MI355X_MICROARCH.md "access shape").
//   * DMA issue moved between the MFMA halves: slower (DMA latency matters more than VALU slots).
//   * 3-wave blocks (192 columns: no padding for Cin = 64 / 128): +3 % at Cin = 64, -5 % at 128 --
//     the padded MFMAs are not on the critical path of this latency-bound loop.
// PMC (256^2 x 64ch): ~48 % of wave cycles in s_waitcnt/barrier, i.e. latency-bound on x/dY
// streamed from HBM with only one K step of lookahead.
#include "bn_dev.h"
#include "rdp_api.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>

struct WgradArgs {
  const u16* x1;
  const u16* x2;
  uint32_t xbytes1, xbytes2;
  int C1, C2, pitch1, pitch2;
  const u16* dy;
  uint32_t dybytes;
  int dypitch;
  float* slab;
  int H, W, M, Cout, Cin;
  int taps, packed;
  int ncols, ncols_pad;
  int colTiles, coutTiles, splits;
  int pix_per_split;
  uint32_t fw_m, fw_s, fh_m, fh_s;  // fast div by W and by H
  // UTR (ConvTranspose2d(2, s2) weight gradient, rdp_conv_wgrad_upT): x1 = the output gradient du
  // [N][uH2][uW2][C1], read at the 4 sub-pixels (2h + tap/2 + uoy, 2w + tap%2 + uox) of low-res
  // pixel (h, w) -- the "taps" -- instead of an unshuffled [N][h][w][4 C1] copy
  int uH2 = 0, uW2 = 0, uoy = 0, uox = 0;
};

RDP_DEV int swz(int p) { return (((p >> 1) & 1) << 1) | (((p >> 3) & 1) << 2); }

// BKP = 64 pixels per K step, double-buffered; 8 waves: waves 2s, 2s+1 split x-subtile s into two
// 32-column halves (twice the waves per SIMD of a 4-wave block, same LDS footprint).
template <bool PACKED, bool UTR = false>
__global__ __launch_bounds__(512, 2) void conv_wgrad_kernel(const WgradArgs a) {
  constexpr bool TILE_FAST = true;
  constexpr int BKP = 64, STAGES = 2, NWV = 8;
  constexpr int SUB = BKP * 128;        // one [BKP pixels][64 ch] bf16 tile
  constexpr int BUF = 5 * SUB;          // 4 x-subtiles + 1 dy tile
  constexpr int PIECES = BKP / 8;       // 8-row DMA pieces per subtile
  constexpr int PPW = PIECES / NWV;     // pieces (row groups) per wave
  constexpr int NI = 4 * 4 / NWV;       // 16-column x fragments per wave (4 or 2)
  static_assert(PPW >= 1, "BKP too small for the wave count");
  __shared__ __attribute__((aligned(16))) char smem[STAGES * BUF];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const uint32_t nwg = gridDim.x;
  const uint32_t lid = xcd_remap(blockIdx.x, nwg);
  // TILE_FAST: consecutive logical ids (same XCD after the remap) = different weight tiles of the
  // SAME pixel range, so they share the dY / X lines in that XCD's L2.
  const int ntiles = a.colTiles * a.coutTiles;
  const int split = TILE_FAST ? lid / ntiles : lid % a.splits;
  const int tile = TILE_FAST ? lid % ntiles : lid / a.splits;
  const int tc = tile % a.colTiles, tn = tile / a.colTiles;
  const int cout0 = tn * 64;
  const int pbeg = split * a.pix_per_split;
  const int pend = min(a.M, pbeg + a.pix_per_split);
  const int nks = (pend - pbeg + BKP - 1) / BKP;

  const auto rx1 = make_rsrc(a.x1, a.xbytes1);
  const auto rx2 = make_rsrc(a.x2 ? a.x2 : a.x1, a.x2 ? a.xbytes2 : 0u);
  const auto rdy = make_rsrc(a.dy, a.dybytes);

  // per-subtile (tap, channel offset, source) -- uniform
  int s_dr[4], s_ds[4], s_ch[4], s_src[4], s_ok[4];
#pragma unroll
  for (int sub = 0; sub < 4; ++sub) {
    const int kc = tc * 256 + sub * 64;
    s_ok[sub] = kc < a.ncols;
    if (PACKED) {
      s_dr[sub] = 0; s_ds[sub] = 0; s_ch[sub] = kc / 8; s_src[sub] = 0;  // s_ch = first tap
    } else {
      const int tap = kc / a.Cin;
      const int cin0 = kc - tap * a.Cin;
      s_dr[sub] = UTR ? tap >> 1 : a.taps == 9 ? tap / 3 - 1 : 0;
      s_ds[sub] = UTR ? tap & 1 : a.taps == 9 ? tap % 3 - 1 : 0;
      s_src[sub] = cin0 >= a.C1;
      s_ch[sub] = s_src[sub] ? cin0 - a.C1 : cin0;
    }
  }

  const int rowl = lane >> 3;  // pixel row within an 8-row DMA piece
  const int cpos = lane & 7;   // 16-B position within the LDS row

  auto issue = [&](int ks, char* buf) {
#pragma unroll
    for (int t = 0; t < PPW; ++t) {
      const int s = wave * PPW + t;  // DMA piece index (8 pixel rows)
      const int p = s * 8 + rowl;  // pixel row in the BKP-pixel K step
      const int g = cpos ^ swz(p);  // global 16-B chunk this lane fetches
      const int m = pbeg + ks * BKP + p;
      const bool mv = m < pend;
      const uint32_t q = fdiv((uint32_t)m, a.fw_m, a.fw_s);
      const int w = m - (int)q * a.W;
      const int h = (int)q - (int)fdiv(q, a.fh_m, a.fh_s) * a.H;
      // dY piece
      {
        const uint32_t off = mv ? (uint32_t)(m * a.dypitch + cout0 + g * 8) * 2u : RDP_OOB;
        dma16_async(rdy, (lds_void*)(buf + 4 * SUB + s * 1024), off);
      }
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        int dr = s_dr[sub], ds = s_ds[sub], ch;
        if constexpr (PACKED) {
          const int tap = s_ch[sub] + g;
          dr = tap / 3 - 1; ds = tap % 3 - 1;
          ch = 0;
          const int hh = h + dr, ww = w + ds;
          const bool ok = mv & (bool)s_ok[sub] & (tap < 9) & inb(hh, a.H) & inb(ww, a.W);
          const uint32_t off = ok ? (uint32_t)((m + dr * a.W + ds) * a.pitch1) * 2u : RDP_OOB;
          dma16_async(rx1, (lds_void*)(buf + sub * SUB + s * 1024), off);
        } else if constexpr (UTR) {  // sub-pixel (dr, ds) of the (2h + uoy, 2w + uox) pixel of du
          ch = s_ch[sub] + g * 8;
          const int img = (int)fdiv(q, a.fh_m, a.fh_s);
          const int px = (img * a.uH2 + 2 * h + a.uoy + dr) * a.uW2 + 2 * w + a.uox + ds;
          const uint32_t off = mv & (bool)s_ok[sub] ? (uint32_t)(px * a.pitch1 + ch) * 2u : RDP_OOB;
          dma16_async(rx1, (lds_void*)(buf + sub * SUB + s * 1024), off);
        } else {
          ch = s_ch[sub] + g * 8;
          const int hh = h + dr, ww = w + ds;
          const bool ok = mv & (bool)s_ok[sub] & inb(hh, a.H) & inb(ww, a.W);
          const int pitch = s_src[sub] ? a.pitch2 : a.pitch1;
          const uint32_t off = ok ? (uint32_t)((m + dr * a.W + ds) * pitch + ch) * 2u : RDP_OOB;
          dma16_async(s_src[sub] ? rx2 : rx1, (lds_void*)(buf + sub * SUB + s * 1024), off);
        }
      }
    }
  };

  f32x4 acc[NI][4];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // transposed-read lane geometry: lane = 16g + 4q + pp
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tpp = lane & 3;

  // one barrier per K step: wait for stage ks (STAGES-2 younger stages stay in flight), the
  // barrier retires every wave's reads of the buffer about to be refilled, then issue ks+STAGES-1.
  constexpr int DMA_PER_STAGE = PPW * 5;
#pragma unroll
  for (int st = 0; st < STAGES - 1; ++st)
    if (st < nks) issue(st, smem + st * BUF);
  for (int ks = 0; ks < nks; ++ks) {
    if constexpr (STAGES == 3) {
      if (ks + 1 < nks) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(DMA_PER_STAGE) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    raw_barrier();
    if (ks + STAGES - 1 < nks) issue(ks + STAGES - 1, smem + ((ks + STAGES - 1) % STAGES) * BUF);
    const char* cur = smem + (ks % STAGES) * BUF;
    const int xsub = NWV == 4 ? wave : (wave >> 1);
    const int i0 = NWV == 4 ? 0 : (wave & 1) * NI;  // first 16-column group of this wave
    const char* xb = cur + xsub * SUB;
    const char* db = cur + 4 * SUB;
#pragma unroll
    for (int hf = 0; hf < BKP / 32; ++hf) {
      bf16x8 fa[NI], fb[4];
      const int p0 = 32 * hf + 8 * tg + tq;
      const int sw0 = swz(p0), sw1 = swz(p0 + 4);
      const int ro0 = p0 * 128 + 8 * (tpp & 1), ro1 = ro0 + 4 * 128;
      typedef __attribute__((address_space(3))) bf16x4 lds_v4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 2 * i + (tpp >> 1);
        const int o0 = ro0 + 16 * (c ^ sw0), o1 = ro1 + 16 * (c ^ sw1);
        const bf16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(db + o0));
        const bf16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(db + o1));
        fb[i] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = 2 * (i0 + i) + (tpp >> 1);
        const int o0 = ro0 + 16 * (c ^ sw0), o1 = ro1 + 16 * (c ^ sw1);
        const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(xb + o0));
        const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(xb + o1));
        fa[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }

  // acc[i][j][r]: col = colbase + 16i + 4*(lane>>4) + r ; cout = cout0 + 16j + (lane&15)
  const int colbase = NWV == 4 ? tc * 256 + wave * 64 : tc * 256 + (wave >> 1) * 64 + (wave & 1) * 32;
  if (colbase >= a.ncols_pad) return;
  const auto rs = make_rsrc(a.slab, (uint32_t)min((long)a.splits * a.Cout * a.ncols_pad * 4l, (long)0x7fffffff));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = cout0 + 16 * j + (lane & 15);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int col = colbase + 16 * i + 4 * (lane >> 4);
      const uint32_t off = (uint32_t)(((long)split * a.Cout + co) * a.ncols_pad + col) * 4u;
      uint4 v;
      v.x = __float_as_uint(acc[i][j][0]); v.y = __float_as_uint(acc[i][j][1]);
      v.z = __float_as_uint(acc[i][j][2]); v.w = __float_as_uint(acc[i][j][3]);
      bstore16(rs, off, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Halo-reuse weight gradient for 3x3 convs whose pixels split into 64-pixel segments of whole rows
// or of one row (W % 64 == 0, or W | 64 with H * W % 64 == 0: every U-Net layer at 256^2..16^2).
//
// The generic kernel above stages one [64 px][64 ch] x tile per (tap, cin-chunk) column subtile,
// i.e. the same input pixels 9 times (once per tap) and 40 KB of DMA per 2 MFLOP. Here one K step
// is one 64-pixel segment (h, w0..w0+63) of one image (or 64 / W whole rows), and the block owns ALL 9 taps of one
// 64-channel input chunk: it stages the three input rows h-1, h, h+1 over pixels w0-1 .. w0+64
// (66 used of 72 staged rows per region, zero halo from out-of-range offsets) plus the dY segment,
// and every tap (dr, ds) is a row-shifted window (rows ds+1 .. ds+64 of region dr+1) of that one
// image. Per K step: 27 KB of x + 8 KB per 64 couts of dY for 9 x 64 x BN x 64 MACs (2.7x the
// FLOP per staged byte at BN = 64, 3.4x at BN = 128).
//
// Block = BN/16 waves; wave w owns input channels 16*(w&3) .. +15 of the chunk for all 9 taps and
// output channels 64*(w>>2) .. +63: 9 x 4 MFMA 16x16x32 accumulators (144 VGPRs), A fragments of the
// three column shifts formed in registers from one 12-pixel window per (region, half step) read by
// ds_read_b64_tr_b16 (wgrad_win_step below), B fragments from the dY tile (same LDS image and
// swizzle as the generic kernel). Split-K over row segments into the same fp32 slab format, reduced
// by wgrad_reduce_kernel.
struct WgradHaloArgs {
  const u16* x1;
  const u16* x2;
  uint32_t xbytes1, xbytes2;
  int C1, C2, pitch1, pitch2;
  const u16* dy;
  uint32_t dybytes;
  int dypitch;
  float* slab;
  uint32_t slab_bytes;
  int H, W, Cout, ncols;  // ncols = 9 * Cin = slab row length
  int cinTiles, coutTiles, splits, segs_per_split, nseg;
  uint32_t fw_m, fw_s, fh_m, fh_s;
};

// ---- fragment reads of one K step (64 pixels), shared by the halo and the ring kernel ----
//
// Transposed-read lane geometry (see conv_wgrad_kernel): lane = 16 tg + 4 tq + tpp. One
// ds_read_b64_tr_b16 whose 16-lane group addresses pixel rows R + tq leaves pixels R .. R + 3 of the
// lane's channel in the lane, two per dword. The A fragment of column shift sh (tap column ds = sh - 1)
// is the 8 pixels 32 hf + 8 tg + sh + e, e = 0..7, of a region: the three shifts overlap in all but two
// pixels, so a (region, half step) is read ONCE as the 12-pixel window 32 hf + 8 tg + 0..11 (three reads,
// dwords d0..d5) and the shifts are formed in registers: sh 0 = (d0..d3), sh 2 = (d1..d4), sh 1 = the four
// 16-bit funnel shifts between them (one v_perm_b32 each). Highest row read: 32 + 24 + 3 + 8 = 67 < 72 staged
// rows; rows >= 66 are zero fill and land only in d5, which no fragment uses.
//
// Offsets are hoisted: the swizzle reads pixel-row bits 1 and 3 only, so the half step's 32-row offset is
// a constant 4 KB and one set of lane offsets serves both halves (immediates).
struct WgradFragOff {
  int a[3];     // window groups: rows 8 tg + tq + 0 / 4 / 8 of this wave's 16 input channels
  int b[2][4];  // dY: rows 8 tg + tq + 0 / 4 of 16-cout group i
};

RDP_DEV WgradFragOff wgrad_frag_off(int lane, int cf) {
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tpp = lane & 3;
  const int ca = 2 * cf + (tpp >> 1);  // 16-B chunk of this lane's A fragment row (input channels)
  const int q0 = 8 * tg + tq;
  WgradFragOff o;
#pragma unroll
  for (int g = 0; g < 3; ++g) o.a[g] = (q0 + 4 * g) * 128 + 8 * (tpp & 1) + 16 * (ca ^ swz(q0 + 4 * g));
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o.b[g][i] = (q0 + 4 * g) * 128 + 8 * (tpp & 1) + 16 * ((2 * i + (tpp >> 1)) ^ swz(q0 + 4 * g));
  return o;
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
struct WgradWin { u32x2 g[3]; };  // d0..d5: 12 consecutive pixels of one channel

RDP_DEV void wgrad_read_win(WgradWin& w, const char* xb, const WgradFragOff& o) {
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
#pragma unroll
  for (int g = 0; g < 3; ++g)
    w.g[g] = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(xb + o.a[g])));
}

template <int SH>
RDP_DEV bf16x8 wgrad_win_frag(const WgradWin& w) {
  const uint32_t d0 = w.g[0][0], d1 = w.g[0][1], d2 = w.g[1][0], d3 = w.g[1][1], d4 = w.g[2][0];
  u32x4 f;
  if (SH == 0) f = u32x4{d0, d1, d2, d3};
  else if (SH == 2) f = u32x4{d1, d2, d3, d4};
  else
    f = u32x4{__builtin_amdgcn_alignbit(d1, d0, 16), __builtin_amdgcn_alignbit(d2, d1, 16),
              __builtin_amdgcn_alignbit(d3, d2, 16), __builtin_amdgcn_alignbit(d4, d3, 16)};
  return __builtin_bit_cast(bf16x8, f);
}

RDP_DEV bf16x8 wgrad_read_b(const char* db, const WgradFragOff& o, int i) {
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;
  const bf16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(db + o.b[0][i]));
  const bf16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(db + o.b[1][i]));
  return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// One K step: acc[3 r + sh][i] += window(region r, shift sh)^T x dY[16-cout group i] over both 32-pixel
// half steps. The six (half step, region) groups are unrolled with two window sets alternating: group
// g + 1's three reads are issued before group g's 12 MFMAs, and at the half-step boundary (g = 2) each
// dY fragment of the next half is read into the registers of the one it replaces right after that one's
// last MFMA (the MFMAs run cout-group-outer for this), so every LDS round trip runs under the matrix
// cores and the waits in between are counted (LDS returns in order). Only group 0 and the first dY
// fragments wait for a read that nothing covers, once per K step -- they cannot start before the step
// barrier, the buffer is still being filled. The sched_barriers pin that order; without them the
// scheduler sinks every read to its first use. Every accumulator still receives the same products in
// the same (K step, half step) order as a plain shift-by-shift loop.
//
// x0..x2: the three input row regions (dr = -1, 0, +1). zero0 / zero2 (wave-uniform; ring kernel, first /
// last image row, where the neighbouring ring slot holds another column's row) make the dr = -1 / +1
// window the zero padding row it stands for. The step stays one basic block that way: with a branch
// around a region's MFMAs the register allocator no longer keeps each accumulator in place and spills
// all 144 of them, and the extra MFMAs are 2 / (3 H) of the kernel's.
// MULTIROW (W < 64): window pixel p + ds of tap ds = -1 / +1 crosses into the neighbouring image row
// where w = 0 / W - 1; those dY pixels are zero for that tap. This lane holds B rows (pixels)
// 32 hf + 8 tg + e, e = 0..7 (MFMA 16x16x32 B layout), so the masks touch only e = 0 (low half of
// dword 0, sh = 0) and e = 7 (high half of dword 3, sh = 2).
template <bool MULTIROW, bool LEAN = false>
RDP_DEV void wgrad_win_step(f32x4 (&acc)[9][4], const char* x0, const char* x1, const char* x2, const char* db,
                            const WgradFragOff& o, bool zero0, bool zero2, int lane, int W) {
  WgradWin win[2];
  bf16x8 fb[4];
  auto read_group = [&](int g) {
    const int r = g % 3;
    wgrad_read_win(win[g & 1], (r == 0 ? x0 : r == 1 ? x1 : x2) + (g / 3) * 4096, o);
  };
  read_group(0);  // window first, dY fragments in the order of their use: the first MFMAs wait for 5 reads, not 11
#pragma unroll
  for (int i = 0; i < 4; ++i) fb[i] = wgrad_read_b(db, o, i);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = 0; g < 6; ++g) {
    const int hf = g / 3, r = g % 3;
    if (g + 1 < 6) read_group(g + 1);
    __builtin_amdgcn_sched_barrier(0);
    const int pl = 32 * hf + 8 * (lane >> 4);
    uint32_t ml = MULTIROW && (pl & (W - 1)) == 0 ? 0xffff0000u : 0xffffffffu;        // e = 0 has w = 0
    uint32_t mr = MULTIROW && ((pl + 8) & (W - 1)) == 0 ? 0x0000ffffu : 0xffffffffu;  // e = 7 has w = W - 1
    // LEAN (no register room, halo<64, MULTIROW>): hide the masks' values from the compiler per group, or it
    // forms the eight masked copies of the dY fragments once per half step and holds them (32 VGPRs, spills)
    if (MULTIROW && LEAN) asm volatile("" : "+v"(ml), "+v"(mr));
    WgradWin w = win[g & 1];
    if ((r == 0 && zero0) || (r == 2 && zero2)) w.g[0] = w.g[1] = w.g[2] = u32x2{0u, 0u};
    const bf16x8 fa[3] = {wgrad_win_frag<0>(w), wgrad_win_frag<1>(w), wgrad_win_frag<2>(w)};
#pragma unroll
    for (int u = 0; u < 12; ++u) {
      const int i = u / 3, sh = u % 3;
      u32x4 b = __builtin_bit_cast(u32x4, fb[i]);
      if (MULTIROW && sh == 0) b[0] &= ml;
      if (MULTIROW && sh == 2) b[3] &= mr;
      acc[3 * r + sh][i] =
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[sh], __builtin_bit_cast(bf16x8, b), acc[3 * r + sh][i], 0, 0, 0);
      if (g == 2 && sh == 2) {  // last use of this half's fb[i]: the next half's goes out under the remaining MFMAs
        __builtin_amdgcn_sched_barrier(0);
        fb[i] = wgrad_read_b(db + 4096, o, i);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// K loop: wait for the staged buffer + barrier, issue the next stage's DMA, then wgrad_win_step above: 34
// transposed reads (was 52: two per shift) and one full lgkmcnt(0) per K step (was 18, one in front of
// every 4 MFMAs with the A fragment in a single reused register quad); numbers before / after in
// profiles/wgrad_frag_pipeline.md. (Measured dead ends, profiles/dead_ends.md: a staggered two-group
// schedule and a 3-stage ring of this kernel. Its ablations -- 535 us full, 382 without the DMA stream,
// 381 without the MFMAs, 344 with neither -- put most of the time in the loop skeleton, not in either
// stream: the exposed fragment-read round trips this loop no longer has were part of it.)
template <int BN, bool MULTIROW>
__global__ __launch_bounds__(BN * 4, 2) void conv_wgrad_halo_kernel(const WgradHaloArgs a) {
  constexpr int STAGES = 2;
  constexpr int NWV = BN / 16;
  constexpr int XREG = 72 * 128;                  // one staged input row region (72 pixel rows x 64 ch)
  constexpr int DSUB = 64 * 128;                  // one [64 px][64 cout] dY subtile
  constexpr int BUF = 3 * XREG + (BN / 64) * DSUB;
  constexpr int XPIECES = 27, NPIECES = XPIECES + 8 * (BN / 64);
  constexpr int PPW = (NPIECES + NWV - 1) / NWV;  // DMA pieces (8 rows x 128 B) per wave per stage
  __shared__ __attribute__((aligned(16))) char smem[STAGES * BUF];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  const uint32_t lid = xcd_remap(blockIdx.x, gridDim.x);
  // consecutive logical ids (one XCD) = different weight tiles of the same segment range: they
  // share the dY / x lines in that XCD's L2
  const int ntiles = a.cinTiles * a.coutTiles;
  const int split = lid / ntiles, tile = lid - split * ntiles;
  const int tc = tile % a.cinTiles, tn = tile / a.cinTiles;
  const int cin0 = tc * 64, cout0 = tn * BN;
  const int s0 = split * a.segs_per_split;
  const int s1 = min(a.nseg, s0 + a.segs_per_split);
  const int nks = s1 - s0;

  const bool src2 = cin0 >= a.C1;
  const auto rx = src2 ? make_rsrc(a.x2, a.xbytes2) : make_rsrc(a.x1, a.xbytes1);
  const int pitch = src2 ? a.pitch2 : a.pitch1;
  const int ch0 = src2 ? cin0 - a.C1 : cin0;
  const auto rdy = make_rsrc(a.dy, a.dybytes);

  const int rowl = lane >> 3, cpos = lane & 7;

  auto issue = [&](int ks, char* buf) {
    const int m0 = (s0 + ks) * 64;  // first pixel of the segment
    const uint32_t q = fdiv((uint32_t)m0, a.fw_m, a.fw_s);
    const int w0 = m0 - (int)q * a.W;
    const int h = (int)q - (int)fdiv(q, a.fh_m, a.fh_s) * a.H;
#pragma unroll
    for (int t = 0; t < PPW; ++t) {
      const int piece = wave + t * NWV;  // wave-uniform
      if (piece < XPIECES) {
        const int r = piece / 9, pj = piece - r * 9;  // region (dr + 1), 8-row piece in the region
        const int j = pj * 8 + rowl;                  // staged row: pixel w0 - 1 + j of image row h + dr
        const int g = cpos ^ swz(j);
        // image row of the staged pixel: row h + dr + floor((w0 - 1 + j) / W). Wide rows (W >= 64)
        // keep only pixels of row h + dr (the rest is the zero halo); multi-row segments (W | 64)
        // keep every in-image row and mask the row-crossing taps on the dY side instead.
        const int wj = w0 - 1 + j;
        const int wq = wj < 0 ? -1 : (int)fdiv((uint32_t)wj, a.fw_m, a.fw_s);
        const bool ok = (j < 66) & (MULTIROW || wq == 0) & inb(h + r - 1 + wq, a.H);
        const uint32_t off = ok ? (uint32_t)((m0 + (r - 1) * a.W + j - 1) * pitch + ch0 + g * 8) * 2u : RDP_OOB;
        dma16_async(rx, (lds_void*)(buf + r * XREG + pj * 1024), off);
      } else if (piece < NPIECES) {
        const int d = piece - XPIECES, sub = d >> 3, pj = d & 7;
        const int p = pj * 8 + rowl;
        const int g = cpos ^ swz(p);
        const uint32_t off = (uint32_t)((m0 + p) * a.dypitch + cout0 + sub * 64 + g * 8) * 2u;
        dma16_async(rdy, (lds_void*)(buf + 3 * XREG + sub * DSUB + pj * 1024), off);
      }
    }
  };

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int cf = wave & 3, cg = wave >> 2;
  const WgradFragOff fo = wgrad_frag_off(lane, cf);

#pragma unroll
  for (int st = 0; st < STAGES - 1; ++st)
    if (st < nks) issue(st, smem + st * BUF);
  // pieces this wave issues per stage (wave-uniform): PPW or PPW - 1
  for (int ks = 0; ks < nks; ++ks) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    raw_barrier();
    if (ks + STAGES - 1 < nks) issue(ks + STAGES - 1, smem + ((ks + STAGES - 1) % STAGES) * BUF);
    const char* cur = smem + (ks % STAGES) * BUF;
    wgrad_win_step<MULTIROW, MULTIROW && BN == 64>(acc, cur, cur + XREG, cur + 2 * XREG, cur + 3 * XREG + cg * DSUB, fo, false, false, lane, a.W);
  }

  // acc[tap][i][r]: cin = cin0 + 16 cf + 4 (lane >> 4) + r, cout = cout0 + 64 cg + 16 i + (lane & 15)
  const auto rs = make_rsrc(a.slab, a.slab_bytes);
  const int cin = cin0 + 16 * cf + 4 * (lane >> 4);
  const int Cin = a.ncols / 9;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = cout0 + 64 * cg + 16 * i + (lane & 15);
    const long rowbase = ((long)split * a.Cout + co) * a.ncols + cin;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint32_t off = (uint32_t)(rowbase + t * Cin) * 4u;
      uint4 v;
      v.x = __float_as_uint(acc[t][i][0]); v.y = __float_as_uint(acc[t][i][1]);
      v.z = __float_as_uint(acc[t][i][2]); v.w = __float_as_uint(acc[t][i][3]);
      bstore16(rs, off, v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Row-ring variant of the halo wgrad for wide rows (W % 64 == 0). K steps walk each 64-pixel
// column (image n, segment wseg) top to bottom: position P = column * H + h. Step P needs input
// rows P - 1, P, P + 1, and rows P - 1 and P were staged by the two previous steps, so a step
// stages ONE new input row region (9 KB) plus its dY tile instead of three regions: half the DMA
// bytes of conv_wgrad_halo_kernel at BN = 64. Input rows live in a 5-slot ring (slot = P % 5), dY
// in a 3-slot ring; two steps stay in flight across the per-step barrier (counted vmcnt). At a
// column's first / last row the dr = -1 / +1 window is zeroed in registers (the neighbouring ring slot
// holds another column's row: that is the zero padding row of this one).
struct WgradRingArgs {
  const u16* x1;
  const u16* x2;
  uint32_t xbytes1, xbytes2;
  int C1, C2, pitch1, pitch2;
  const u16* dy;
  uint32_t dybytes;
  int dypitch;
  float* slab;
  uint32_t slab_bytes;
  int H, W, Cout, ncols;
  int cinTiles, coutTiles, splits, pos_per_split, npos;
  int WS;                           // 64-pixel segments per image row
  uint32_t fh_m, fh_s, fs_m, fs_s;  // fast div by H and by WS
};

template <int BN>
__global__ __launch_bounds__(BN * 4, 2) void conv_wgrad_ring_kernel(const WgradRingArgs a) {
  constexpr int NWV = BN / 16;
  constexpr int XREG = 72 * 128;   // one staged input row region: pixels w0-1 .. w0+70 (66 used)
  constexpr int DSUB = 64 * 128;   // [64 px][64 cout] dY subtile
  constexpr int NX = 5, ND = 3;    // ring slots
  constexpr int DT = (BN / 64) * DSUB;
  constexpr int XPIECES = 9, NPIECES = XPIECES + 8 * (BN / 64);
  constexpr int PPW = (NPIECES + NWV - 1) / NWV;
  constexpr int MINPW = NPIECES / NWV;  // DMAs issued per step by the wave that issues fewest
  __shared__ __attribute__((aligned(16))) char smem[NX * XREG + ND * DT];
  char* const xring = smem;
  char* const dring = smem + NX * XREG;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t lid = xcd_remap(blockIdx.x, gridDim.x);
  const int ntiles = a.cinTiles * a.coutTiles;
  const int split = lid / ntiles, tile = lid - split * ntiles;
  const int tc = tile % a.cinTiles, tn = tile / a.cinTiles;
  const int cin0 = tc * 64, cout0 = tn * BN;
  const int p0s = split * a.pos_per_split;
  const int nks = min(a.npos, p0s + a.pos_per_split) - p0s;

  const bool src2 = cin0 >= a.C1;
  const auto rx = src2 ? make_rsrc(a.x2, a.xbytes2) : make_rsrc(a.x1, a.xbytes1);
  const int pitch = src2 ? a.pitch2 : a.pitch1;
  const int ch0 = src2 ? cin0 - a.C1 : cin0;
  const auto rdy = make_rsrc(a.dy, a.dybytes);
  const int rowl = lane >> 3, cpos = lane & 7;

  // position -> (first pixel of the segment, row h); P may be -1 or npos (loads read zeros)
  auto locate = [&](int P, int& m0, int& h, int& w0) {
    const uint32_t up = (uint32_t)max(P, 0);
    const uint32_t col = fdiv(up, a.fh_m, a.fh_s);
    h = (int)(up - col * (uint32_t)a.H);
    const uint32_t n = fdiv(col, a.fs_m, a.fs_s);
    const int wseg = (int)(col - n * (uint32_t)a.WS);
    m0 = (((int)n * a.H + h) * a.WS + wseg) * 64;
    w0 = wseg * 64;
    if (P < 0 || P >= a.npos) h = -2;  // no such row: every pixel out of the image
  };
  // piece t of this wave: x-row pieces (when wx) then dY pieces (when wd)
  auto issue = [&](int P, bool wx, bool wd) {
    int m0, h, w0;
    locate(P, m0, h, w0);
#pragma unroll
    for (int t = 0; t < PPW; ++t) {
      const int piece = wave + t * NWV;
      if (piece < XPIECES) {
        if (!wx) continue;
        const int j = piece * 8 + rowl;
        const int g = cpos ^ swz(j);
        const bool ok = (j < 66) & inb(w0 - 1 + j, a.W) & inb(h, a.H);
        const uint32_t off = ok ? (uint32_t)((m0 + j - 1) * pitch + ch0 + g * 8) * 2u : RDP_OOB;
        dma16_async(rx, (lds_void*)(xring + ((P + NX) % NX) * XREG + piece * 1024), off);
      } else if (piece < NPIECES) {
        if (!wd) continue;
        const int d = piece - XPIECES, sub = d >> 3, pj = d & 7;
        const int p = pj * 8 + rowl;
        const int g = cpos ^ swz(p);
        const bool ok = inb(h, a.H);
        const uint32_t off = ok ? (uint32_t)((m0 + p) * a.dypitch + cout0 + sub * 64 + g * 8) * 2u : RDP_OOB;
        dma16_async(rdy, (lds_void*)(dring + (((P - p0s) % ND) * DT) + sub * DSUB + pj * 1024), off);
      }
    }
  };

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int cf = wave & 3, cg = wave >> 2;
  const WgradFragOff fo = wgrad_frag_off(lane, cf);

  // prologue: rows P0 - 1, P0 (x only), then steps 0 and 1 (row P + 1 and dY P)
  if (nks > 0) {
    issue(p0s - 1, true, false);
    issue(p0s, true, false);
    issue(p0s + 1, true, false);
    issue(p0s, false, true);
    if (nks > 1) { issue(p0s + 2, true, false); issue(p0s + 1, false, true); }
  }
  for (int ks = 0; ks < nks; ++ks) {
    const int P = p0s + ks;
    // step ks's data: everything but the (up to MINPW-per-wave) DMAs of step ks + 1
    if (ks + 1 < nks) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(MINPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    raw_barrier();
    if (ks + 2 < nks) { issue(P + 3, true, false); issue(P + 2, false, true); }
    int m0, h, w0;
    locate(P, m0, h, w0);
    const bool top = h == 0, bottom = h == a.H - 1;
    const char* x0 = xring + ((P - 1 + NX) % NX) * XREG;
    const char* x1 = xring + ((P + NX) % NX) * XREG;
    const char* x2 = xring + ((P + 1 + NX) % NX) * XREG;
    const char* db = dring + ((ks % ND) * DT) + cg * DSUB;
    wgrad_win_step<false>(acc, x0, x1, x2, db, fo, top, bottom, lane, a.W);
  }

  const auto rs = make_rsrc(a.slab, a.slab_bytes);
  const int cin = cin0 + 16 * cf + 4 * (lane >> 4);
  const int Cin = a.ncols / 9;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = cout0 + 64 * cg + 16 * i + (lane & 15);
    const long rowbase = ((long)split * a.Cout + co) * a.ncols + cin;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint32_t off = (uint32_t)(rowbase + t * Cin) * 4u;
      uint4 v;
      v.x = __float_as_uint(acc[t][i][0]); v.y = __float_as_uint(acc[t][i][1]);
      v.z = __float_as_uint(acc[t][i][2]); v.w = __float_as_uint(acc[t][i][3]);
      bstore16(rs, off, v);
    }
  }
}

// Split-K slab reduction, two levels. A layer's slab is [splits][Cout][ncols_pad] fp32 with up to
// ~500-2000 splits but often only a few 10^4 elements per split (64 x 576 for a 64 -> 64 layer):
// one thread per output walking all splits left ~150 blocks, each latency-bound on a long chain of
// loads (412 us for 75 MB on inc.double_conv.3 at bs64, at the very end of backward). Level 1 sums
// G contiguous groups of splits into the group's first row in place (~1000 blocks, 16-B loads, 4
// independent accumulators); level 2 sums the G group rows into the weight-gradient layout.

// slab rows s0(g) = g * splits / G (g < G) become sum_{s in [s0(g), s0(g+1))} slab[s]
__global__ __launch_bounds__(256) void wgrad_group_sum_kernel(float* __restrict__ slab, long E, int splits, int G) {
  const long e4 = (long)blockIdx.x * 256 + threadIdx.x;  // float4 index within one split row
  if (e4 * 4 >= E) return;
  const int g = blockIdx.y;
  const int s0 = (int)((long)g * splits / G), s1 = (int)((long)(g + 1) * splits / G);
  const float4* p = (const float4*)slab + e4;
  const long st = E >> 2;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  int sp = s0;
  for (; sp + 4 <= s1; sp += 4) {
    const float4 v0 = p[(long)sp * st], v1 = p[(long)(sp + 1) * st], v2 = p[(long)(sp + 2) * st],
                 v3 = p[(long)(sp + 3) * st];
    a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
    a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
    a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
  }
  for (; sp < s1; ++sp) {
    const float4 v = p[(long)sp * st];
    a0.x += v.x; a0.y += v.y; a0.z += v.z; a0.w += v.w;
  }
  ((float4*)slab)[(long)s0 * st + e4] = make_float4((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y),
                                                    (a0.z + a1.z) + (a2.z + a3.z), (a0.w + a1.w) + (a2.w + a3.w));
}

// out[cout][tap][cin_real] (+)= sum_g slab[s0(g)][cout][tap*cin_pad + cin]   (s0(g) = g * splits / G)
// V = 4 (cin_real % 4 == 0): each thread owns 4 consecutive outputs, 16-B slab loads / stores (same
// per-element summation order as V = 1; bs 4 step 2.40 -> 2.38 ms)
template <int V>
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, int splits, int G, int Cout,
                                    int ncols_pad, int taps, int cin_pad, int cin_real, int accumulate) {
  typedef float vf __attribute__((ext_vector_type(V)));
  const long total = (long)Cout * taps * cin_real / V;
  const long stride = (long)Cout * ncols_pad;
  for (long iv = blockIdx.x * (long)blockDim.x + threadIdx.x; iv < total; iv += (long)gridDim.x * blockDim.x) {
    const long idx = iv * V;
    const int cin = idx % cin_real;
    const long t2 = idx / cin_real;
    const int tap = t2 % taps;
    const int co = t2 / taps;
    const long col = (long)tap * cin_pad + cin;
    const float* p = slab + (long)co * ncols_pad + col;
    // 8 independent accumulators: the row loop is latency-bound otherwise
    vf s[8] = {};
    int g = 0;
    for (; g + 8 <= G; g += 8)
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += *(const vf*)(p + ((long)(g + u) * splits / G) * stride);
    for (; g < G; ++g) s[0] += *(const vf*)(p + ((long)g * splits / G) * stride);
    const vf r = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    *(vf*)(out + idx) = accumulate ? *(const vf*)(out + idx) + r : r;
  }
}

// RDP_ABLATE (profiling only, wrong results): "wgsum" skips the level-1 group sums, "wgred" both levels
static int ablate_flags() {
  static const int f = [] {
    const char* v = getenv("RDP_ABLATE");
    if (!v) return 0;
    return (strstr(v, "wgsum") ? 1 : 0) | (strstr(v, "wgred") ? 2 : 0);
  }();
  return f;
}

// The two-level reduce of a planned weight gradient's slab into g.out (geometry: rdp_wgrad_reduce_geo)
void rdp_wgrad_reduce(const RdpWgrad& g, const RdpWgradPlan& p, hipStream_t s) {
  if (ablate_flags() & 2) return;
  const RdpWgradReduce& r = p.reduce;
  const long E = (long)p.Cout * p.ncols_pad;
  if (r.grid1 && !(ablate_flags() & 1))
    hipLaunchKernelGGL(wgrad_group_sum_kernel, dim3(r.grid1, r.G), dim3(256), 0, s, g.slab, E, p.splits, r.G);
  if (r.vec == 4)
    hipLaunchKernelGGL(wgrad_reduce_kernel<4>, dim3(r.grid2), dim3(256), 0, s, g.slab, g.out, p.splits, r.G, p.Cout,
                       p.ncols_pad, p.taps, p.cin_pad, p.cin_out, g.accumulate);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3(r.grid2), dim3(256), 0, s, g.slab, g.out, p.splits, r.G, p.Cout,
                       p.ncols_pad, p.taps, p.cin_pad, p.cin_out, g.accumulate);
}

// the fields WgradArgs, WgradHaloArgs and WgradRingArgs share
template <class Args>
static void wgrad_operands(Args& a, const RdpWgrad& g) {
  a.x1 = (const u16*)g.x1; a.x2 = (const u16*)g.x2;
  a.xbytes1 = (uint32_t)g.xbytes1; a.xbytes2 = (uint32_t)g.xbytes2;
  a.C1 = g.C1; a.C2 = g.C2; a.pitch1 = g.pitch1; a.pitch2 = g.pitch2;
  a.dy = (const u16*)g.dy; a.dybytes = (uint32_t)g.dybytes; a.dypitch = g.dypitch;
  a.slab = g.slab; a.H = g.H; a.W = g.W; a.Cout = g.Cout;
}

// conv_wgrad_kernel's arguments for a plan of the generic family (GENERIC, PACKED, UPT)
static WgradArgs wgrad_generic_args(const RdpWgrad& g, const RdpWgradPlan& p) {
  WgradArgs a;
  wgrad_operands(a, g);
  a.M = g.N * g.H * g.W; a.Cin = p.cin_pad;
  a.taps = g.taps; a.packed = g.packed;
  a.ncols = p.ncols; a.ncols_pad = p.ncols_pad;
  a.colTiles = p.ncols_pad / 256; a.coutTiles = g.Cout / 64;
  a.splits = p.splits; a.pix_per_split = p.per_split;
  const FastDiv fw = make_fastdiv(g.W), fh = make_fastdiv(g.H);
  a.fw_m = fw.m; a.fw_s = fw.s; a.fh_m = fh.m; a.fh_s = fh.s;
  return a;
}

int rdp_conv_wgrad(const RdpWgrad& g, int kernel, int splits, hipStream_t s) {
  const RdpWgradPlan p = rdp_wgrad_plan(g, kernel, splits);
  if (p.status != RDP_WGRAD_OK) return p.status;
  const FastDiv fw = make_fastdiv(g.W), fh = make_fastdiv(g.H);
  switch (p.kernel) {
    case RDP_WGRAD_RING: {
      WgradRingArgs a;
      wgrad_operands(a, g);
      a.slab_bytes = (uint32_t)(p.slab_elems * 4); a.ncols = p.ncols;
      a.cinTiles = p.cin_pad / 64; a.coutTiles = g.Cout / p.BN; a.splits = p.splits;
      a.pos_per_split = p.per_split; a.npos = g.N * g.H * g.W / 64; a.WS = g.W / 64;
      const FastDiv fs = make_fastdiv(g.W / 64);
      a.fh_m = fh.m; a.fh_s = fh.s; a.fs_m = fs.m; a.fs_s = fs.s;
      hipLaunchKernelGGL((conv_wgrad_ring_kernel<64>), dim3(p.grid), dim3(p.block), 0, s, a);
      break;
    }
    case RDP_WGRAD_HALO: {
      WgradHaloArgs a;
      wgrad_operands(a, g);
      a.slab_bytes = (uint32_t)(p.slab_elems * 4); a.ncols = p.ncols;
      a.cinTiles = p.cin_pad / 64; a.coutTiles = g.Cout / p.BN; a.splits = p.splits;
      a.segs_per_split = p.per_split; a.nseg = g.N * g.H * g.W / 64;
      a.fw_m = fw.m; a.fw_s = fw.s; a.fh_m = fh.m; a.fh_s = fh.s;
      if (p.BN == 128 && p.multirow) hipLaunchKernelGGL((conv_wgrad_halo_kernel<128, true>), dim3(p.grid), dim3(p.block), 0, s, a);
      else if (p.BN == 128) hipLaunchKernelGGL((conv_wgrad_halo_kernel<128, false>), dim3(p.grid), dim3(p.block), 0, s, a);
      else if (p.multirow) hipLaunchKernelGGL((conv_wgrad_halo_kernel<64, true>), dim3(p.grid), dim3(p.block), 0, s, a);
      else hipLaunchKernelGGL((conv_wgrad_halo_kernel<64, false>), dim3(p.grid), dim3(p.block), 0, s, a);
      break;
    }
    case RDP_WGRAD_PACKED:
      hipLaunchKernelGGL((conv_wgrad_kernel<true>), dim3(p.grid), dim3(p.block), 0, s, wgrad_generic_args(g, p));
      break;
    case RDP_WGRAD_GENERIC:
      hipLaunchKernelGGL((conv_wgrad_kernel<false>), dim3(p.grid), dim3(p.block), 0, s, wgrad_generic_args(g, p));
      break;
    default: return RDP_WGRAD_NO_FIT;
  }
  rdp_wgrad_reduce(g, p, s);
  return p.splits;
}

int rdp_conv_wgrad_upT(const RdpWgrad& g, const RdpUpT& t, int splits, hipStream_t s) {
  const RdpWgradPlan p = rdp_wgrad_plan(g, RDP_WGRAD_AUTO, splits, t);
  if (p.status != RDP_WGRAD_OK) return p.status;
  WgradArgs a = wgrad_generic_args(g, p);
  a.pitch2 = g.pitch1;
  a.uH2 = t.H2; a.uW2 = t.W2; a.uoy = t.oy; a.uox = t.ox;
  hipLaunchKernelGGL((conv_wgrad_kernel<false, true>), dim3(p.grid), dim3(p.block), 0, s, a);
  rdp_wgrad_reduce(g, p, s);
  return p.splits;
}

// ---------------------------------------------------------------------------------------------
// First layer (inc.double_conv.0, 3 -> 64, reference /root/reference/pkg/segmentation_model.py:31):
// BN-backward apply + ReLU mask fused into the weight gradient. The first conv has no input
// gradient, so its pre-BN gradient dz = A * relu_mask(y) * da + B * y + K (the bn_relu_bwd_apply
// formula, norm_act.hip) is consumed ONLY by this wgrad: computing it here, in registers, and staging
// it straight into the LDS dY tile drops the 537 MB dz write + re-read of a bs-64 step (the separate
// apply pass plus the packed wgrad's dY stream) at the end of backward, where it sits on the
// critical path.
//
// Per 64-pixel K step a block stages: x taps 0..7 (8 channels each, channel 3..7 the stored zero pad)
// and tap 8 by LDS-DMA (the packed layout of conv_wgrad_kernel<PACKED>), and dz [64 px][64 couts]
// computed from da / y by every thread (channel group tc = tid & 7 fixed per thread, so the 40
// BN coefficients stay in registers; swizzle applied on the LDS write address). Only the 80 valid
// (tap, channel) columns are multiplied (5 MFMA column fragments instead of the packed kernel's 16).
// Wave w owns couts 16w .. 16w + 15. The dz loads of step k + 1 are issued before step k's MFMAs and
// written to the other LDS buffer after them (one barrier per step). Slab [splits][64][80] fp32,
// reduced by the shared two-level wgrad reduction.
struct FirstWgradArgs {
  const u16* x;
  uint32_t xbytes;
  int xpitch;
  const u16* da;
  uint32_t dabytes;
  int dapitch;
  const u16* y;
  uint32_t ybytes;
  int ypitch;
  const float* coef;   // [mean | invstd | scale | shift] x 64
  const float* coef2;  // [A | B | K] x 64 (bn_bwd_finalize)
  float* slab;
  uint32_t slab_bytes;
  int H, W, M, pix_per_split;
  uint32_t fw_m, fw_s, fh_m, fh_s;
};
constexpr int FWG_NCOLS = RDP_WGRAD_FIRST_NCOLS;

__global__ __launch_bounds__(256, 2) void wgrad_first_bn_kernel(const FirstWgradArgs a) {
  constexpr int SUB = 64 * 128;  // [64 px][64 bf16]
  constexpr int BUF = 3 * SUB;   // x taps 0..7 | x tap 8 | dz
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int split = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int pbeg = split * a.pix_per_split;
  const int nks = max(0, min(a.M, pbeg + a.pix_per_split) - pbeg) / 64;  // host: multiples of 64
  const auto rx = make_rsrc(a.x, a.xbytes);
  const auto rda = make_rsrc(a.da, a.dabytes);
  const auto ry = make_rsrc(a.y, a.ybytes);

  // dz producer role: channel group tc (fixed), pixel rows tr0 and tr0 + 32 of each K step
  const int tc = threadIdx.x & 7, tr0 = threadIdx.x >> 3;
  float ss[8], hh[8], cA[8], cB[8], cK[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = 8 * tc + k;
    ss[k] = a.coef[bn_off(BN_SCALE, 64) + c]; hh[k] = a.coef[bn_off(BN_SHIFT, 64) + c];
    cA[k] = a.coef2[bn_off(BN2_A, 64) + c]; cB[k] = a.coef2[bn_off(BN2_B, 64) + c];
    cK[k] = a.coef2[bn_off(BN2_K, 64) + c];
  }
  uint4 vd[2], vy[2];
  auto load_dz = [&](int ks) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = pbeg + ks * 64 + tr0 + 32 * u;
      vd[u] = bload16(rda, (uint32_t)(m * a.dapitch + 8 * tc) * 2u);
      vy[u] = bload16(ry, (uint32_t)(m * a.ypitch + 8 * tc) * 2u);
    }
  };
  auto store_dz = [&](char* buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int p = tr0 + 32 * u;
      float fd[8], fy[8];
      unpack8(vd[u], fd);
      unpack8(vy[u], fy);
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 8; k += 2) {
        const float g0 = bn_relu_grad(fd[k], fy[k], ss[k], hh[k]);
        const float g1 = bn_relu_grad(fd[k + 1], fy[k + 1], ss[k + 1], hh[k + 1]);
        o[k / 2] = pack2bf(bn_bwd_apply(g0, fy[k], cA[k], cB[k], cK[k]),
                           bn_bwd_apply(g1, fy[k + 1], cA[k + 1], cB[k + 1], cK[k + 1]));
      }
      *(uint4*)(buf + 2 * SUB + p * 128 + 16 * (tc ^ swz(p))) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  };
  const int rowl = lane >> 3, cpos = lane & 7;
  // x: 16 DMA pieces (2 subtiles x 8 pieces of 8 pixel rows), 4 per wave
  auto issue_x = [&](int ks, char* buf) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int s = wave * 4 + t, sub = s >> 3, pj = s & 7;
      const int p = pj * 8 + rowl;
      const int g = cpos ^ swz(p);
      const int m = pbeg + ks * 64 + p;
      const uint32_t q = fdiv((uint32_t)m, a.fw_m, a.fw_s);
      const int w = m - (int)q * a.W;
      const int h = (int)q - (int)fdiv(q, a.fh_m, a.fh_s) * a.H;
      const int tap = sub * 8 + g;
      const int dr = tap / 3 - 1, ds = tap % 3 - 1;
      const bool ok = (tap < 9) & inb(h + dr, a.H) & inb(w + ds, a.W);
      const uint32_t off = ok ? (uint32_t)((m + dr * a.W + ds) * a.xpitch) * 2u : RDP_OOB;
      dma16_async(rx, (lds_void*)(buf + sub * SUB + pj * 1024), off);
    }
  };

  f32x4 acc[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int tg = lane >> 4, tq = (lane >> 2) & 3, tpp = lane & 3;
  typedef __attribute__((address_space(3))) bf16x4 lds_v4;

  if (nks > 0) {
    load_dz(0);
    issue_x(0, smem);
    store_dz(smem);
  }
  for (int ks = 0; ks < nks; ++ks) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    raw_barrier();
    const char* cur = smem + (ks & 1) * BUF;
    char* nxt = smem + ((ks + 1) & 1) * BUF;
    const bool more = ks + 1 < nks;
    if (more) {
      load_dz(ks + 1);
      issue_x(ks + 1, nxt);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int p0 = 32 * hf + 8 * tg + tq;
      const int sw0 = swz(p0), sw1 = swz(p0 + 4);
      const int ro0 = p0 * 128 + 8 * (tpp & 1), ro1 = ro0 + 4 * 128;
      auto frag = [&](const char* base, int i) {
        const int c = 2 * i + (tpp >> 1);
        const bf16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(base + ro0 + 16 * (c ^ sw0)));
        const bf16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(base + ro1 + 16 * (c ^ sw1)));
        return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      };
      const bf16x8 fb = frag(cur + 2 * SUB, wave);
      bf16x8 fa[5];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag(cur, i);
      fa[4] = frag(cur + SUB, 0);
#pragma unroll
      for (int i = 0; i < 5; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i], 0, 0, 0);
    }
    if (more) store_dz(nxt);
  }

  // acc[i][r]: col = 16 i + 4 (lane >> 4) + r, cout = 16 wave + (lane & 15)
  const auto rs = make_rsrc(a.slab, a.slab_bytes);
  const int co = 16 * wave + (lane & 15);
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int col = 16 * i + 4 * (lane >> 4);
    const uint32_t off = (uint32_t)(((long)split * 64 + co) * FWG_NCOLS + col) * 4u;
    uint4 v;
    v.x = __float_as_uint(acc[i][0]); v.y = __float_as_uint(acc[i][1]);
    v.z = __float_as_uint(acc[i][2]); v.w = __float_as_uint(acc[i][3]);
    bstore16(rs, off, v);
  }
}

int rdp_wgrad_first_bn(const RdpWgrad& g, const RdpWgradBn& bn, int splits, hipStream_t s) {
  const RdpWgradPlan p = rdp_wgrad_plan(g, RDP_WGRAD_AUTO, splits, RdpUpT{}, bn);
  if (p.status != RDP_WGRAD_OK) return p.status;
  FirstWgradArgs a;
  a.x = (const u16*)g.x1; a.xbytes = (uint32_t)g.xbytes1; a.xpitch = g.pitch1;
  a.da = (const u16*)bn.da; a.dabytes = (uint32_t)bn.dabytes; a.dapitch = bn.dapitch;
  a.y = (const u16*)bn.y; a.ybytes = (uint32_t)bn.ybytes; a.ypitch = bn.ypitch;
  a.coef = bn.coef; a.coef2 = bn.coef2;
  a.slab = g.slab; a.slab_bytes = (uint32_t)(p.slab_elems * 4);
  a.H = g.H; a.W = g.W; a.M = g.N * g.H * g.W; a.pix_per_split = p.per_split;
  const FastDiv fw = make_fastdiv(g.W), fh = make_fastdiv(g.H);
  a.fw_m = fw.m; a.fw_s = fw.s; a.fh_m = fh.m; a.fh_s = fh.s;
  hipLaunchKernelGGL(wgrad_first_bn_kernel, dim3(p.grid), dim3(p.block), 0, s, a);
  rdp_wgrad_reduce(g, p, s);
  return p.splits;
}

