// Implicit-GEMM 3x3 / 1x1 convolution, NHWC bf16, MFMA 16x16x32 (gfx950).
//
// Replaces the cuDNN/MIOpen conv forward the reference reaches through torch eager
// (/root/reference/pkg/segmentation_model.py:31,34 -> nn.Conv2d(k=3, pad=1, bias=False)).
// The same kernel computes conv dgrad (dX = conv(dY, flip(W)^T)) with a pre-transposed weight.
//
// GEMM view: out[m = pixel][n = cout] = sum_k im2col(x)[m][k] * W[n][k], k = (tap, cin).
//   * Two input sources are concatenated along channels (torch.cat([skip, up]) in Up.forward,
//     segmentation_model.py:75) so the concat is never materialised.
//   * Output may be split at channel Cy1 into two destinations (dgrad of the concat input).
//   * Epilogue optionally emits per-channel (sum, sumsq) partials of the bf16-rounded output for
//     training-mode BatchNorm: one slab row per (M tile, wave row), reduced by bn_finalize.
//
// Tiling: block = 4 waves (256 threads), block tile BM x BN with each wave owning 64x64; K step
// = 64 channels of one tap. Both operand tiles are staged global->LDS by LDS-DMA
// (buffer_load ... lds, 16 B/lane) as a row-major [rows][128 B] image: one wave-instruction moves
// 8 full 128-B lines, with the 16-B chunk XOR-swizzled by (row & 7) on the SOURCE address so the
// MFMA-fragment ds_read_b128s are bank-conflict free. (A fragment-shaped image -- 16 rows x 64 B
// per instruction -- doubles the TA line lookups and ran 1.4-1.6x slower on deep layers.)
// Halo/zero padding comes from out-of-range buffer offsets (hardware returns 0).
//
// Persistent: each block walks several output tiles with ONE continuous double-buffered K
// pipeline (one raw s_barrier per K step), so tile t+1's first DMA lands under tile t's last
// MFMAs and epilogue. This removes the per-tile prologue that dominated the small-K (K = 576)
// 64-channel layers. The epilogue uses no LDS and no block barrier.
#include "bn_dev.h"
#include "pool_dev.h"
#include "rdp_api.h"

struct ConvArgs {
  const u16* x1;
  const u16* x2;
  uint32_t xbytes1, xbytes2;
  int C1, C2;  // channels in each source (source 2 may be empty)
  int pitch1, pitch2;  // pixel pitch (elements)
  const u16* w;
  uint32_t wbytes;
  int ldw;  // weight row length (elements) = taps * Cin (padded)
  u16* y1;
  u16* y2;
  uint32_t ybytes1, ybytes2;
  int Cy1;  // channels going to y1 (rest to y2)
  int ypitch1, ypitch2;
  float* stats;  // [tilesM * WAVES_M][2][Cout] partial (sum, sumsq) or nullptr
  const float* escale;  // eval-mode BN fold: out = relu?(acc * escale[n] + eshift[n]) (or nullptr)
  const float* eshift;
  int erelu;
  int N, H, W, Cout, M;
  int taps;  // 9 (3x3) or 1 (1x1)
  int packed;  // 1: Cin == 8, K packs 8 taps per 64-wide K step
  int nks;  // number of K steps per work item (= per tile unless split-K)
  int cpt;  // 64-channel chunks per tap (generic mode)
  int ksplit;    // > 1: split-K, work item = (tile, split), fp32 partial tiles go to kslab
  float* kslab;  // [ksplit][M][Cout] fp32
  u16* pool;       // split-K reduce only: also write MaxPool2d(2) of the output (eval), [M/4][ppitch]
  int ppitch;
  // split-K reduce only: also write the bilinear x2 (align_corners) upsample of the output (eval), into
  // up [N][uH][uW][upitch] at offset (uoy, uox) (F.pad of the decoder), zeros outside
  u16* up;
  int upitch, uH, uW, uoy, uox;
  float urh, urw;
  int tilesN, ntiles;
  uint32_t fhw_m, fhw_s, fw_m, fw_s;  // magic division by H*W and by W
  // ConvTranspose2d(k=2, s=2) output written in place (ping-pong epilogue, rdp_conv_upT_fwd): GEMM
  // column n = sub * 2^tlc + c of low-res pixel (img, h, w) goes to y1 pixel (img, 2h + sub/2 + toy,
  // 2w + sub%2 + tox) of a [N][tH2][tW2] map, channel c, + ubias[c]. tlc = 0: plain output.
  const float* ubias = nullptr;
  int tlc = 0, tH2 = 0, tW2 = 0, toy = 0, tox = 0;
  // split-K reduce only (training dgrad, one destination): the BN-backward partial rows of the BN + ReLU
  // layer whose activation gradient this conv writes, in bn_relu_bwd_reduce's layout -- bnpart[block][0][c]
  // = sum g, [block][1][c] = sum g * xhat, g = out * (bny * scale + shift > 0), xhat = (bny - mean) * invstd
  // -- so the standalone reduce pass (reading the output and bny back) disappears
  const u16* bny = nullptr;       // that layer's pre-BN output
  const float* bncoef = nullptr;  // its [mean | invstd | scale | shift]
  float* bnpart = nullptr;
  int bnypitch = 0;
  int* bnrows = nullptr;  // host cell: the partial rows written (set when the split-K reduce ran)
};

template <int N>
RDP_DEV void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
// wait until at most B + (epilogue stores issued since) vector-memory ops are outstanding
template <int B, int P1, int P2>
RDP_DEV void vm_wait_p(int pend) {
  if (pend == 0) vm_wait<B>();
  else if (pend == P1) vm_wait<B + P1>();
  else vm_wait<B + P2>();
}

// Double-buffered K pipeline at 2 blocks / CU: the co-resident block hides the DMA latency. (A 3-4
// stage ring at 1 block / CU and an in-kernel split-K fixup were measured slower: profiles/dead_ends.md.)
template <int BM, int BN, int NWV = 4>
__global__ __launch_bounds__(64 * NWV, 2) void conv_igemm_kernel(const ConvArgs a) {
  constexpr int NST = 2;
  constexpr int WAVES_M = BM / 64;
  constexpr int WAVES_N = NWV / WAVES_M;
  constexpr int WNT = BN / WAVES_N;  // couts per wave (64, or 32 with 8-wave blocks)
  constexpr int NJ = WNT / 16;
  constexpr int P_BYTES = BM * 128, W_BYTES = BN * 128, BUF = P_BYTES + W_BYTES;
  constexpr int NROW = BM / 8 / NWV;     // pixel-row DMA pieces per wave per K step
  constexpr int WPIECES = BN / 8 / NWV;  // weight-row DMA pieces per wave per K step
  constexpr int DMA_OPS = NROW + WPIECES;  // vector-memory ops per wave per stage
  __shared__ __attribute__((aligned(16))) char smem[NST * BUF];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const int gch = (lane & 7) ^ (lane >> 3);  // global 16-B chunk this lane fetches (row-major image)

  const uint32_t G = gridDim.x;
  const uint32_t lid = xcd_remap(blockIdx.x, G);
  const int my_tiles = lid < (uint32_t)a.ntiles ? (a.ntiles - 1 - (int)lid) / (int)G + 1 : 0;
  const int total = my_tiles * a.nks;

  const auto rx1 = make_rsrc(a.x1, a.xbytes1);
  const auto rx2 = make_rsrc(a.x2 ? a.x2 : a.x1, a.x2 ? a.xbytes2 : 0u);
  const auto rw = make_rsrc(a.w, a.wbytes);

  // ---- DMA-side state of the tile currently being staged ----
  // per pixel row (computed once per tile): byte offset of this lane's 16-B chunk of the pixel in
  // each source (pb1 / pb2), and the INVERTED 9-bit tap mask (bit t set <=> row invalid or
  // (h+dr, w+ds) outside the image). The per-K-step address is then 3 full-rate VALU ops per DMA:
  // v_bfe (tap bit) + v_add (uniform tap/channel offset) + v_lshl_or (bit 31 = out of range, which
  // the buffer descriptor turns into zeros) -- no multiply or compare in the K loop.
  uint32_t pb1[NROW], pb2[NROW];
  uint32_t nmask[NROW];
  uint32_t woff[WPIECES];
  int itap = 0, icc = 0;  // (tap, 64-channel chunk) of the stage being issued (generic mode)
  int ks0 = 0;  // first global K step of the work item being staged (split-K)
  auto set_tile = [&](int t) {
    const int item = (int)lid + t * (int)G;
    const int tile = a.ksplit > 1 ? item % (a.ntiles / a.ksplit) : item;
    ks0 = a.ksplit > 1 ? (item / (a.ntiles / a.ksplit)) * a.nks : 0;
    itap = ks0 / a.cpt;
    icc = ks0 - itap * a.cpt;
    const int tm = tile / a.tilesN, tn = tile - tm * a.tilesN;
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
      const int m = tm * BM + (wave * NROW + r) * 8 + (lane >> 3);
      const bool valid = m < a.M;
      const uint32_t mm = valid ? (uint32_t)m : 0u;
      const uint32_t hw = mm - ((__umulhi(mm, a.fhw_m) + mm) >> a.fhw_s) * (uint32_t)(a.H * a.W);
      const uint32_t h = (__umulhi(hw, a.fw_m) + hw) >> a.fw_s;
      const uint32_t w = hw - h * (uint32_t)a.W;
      // rows allowed: dr=-1 needs h>0, dr=+1 needs h<H-1; same for columns
      const uint32_t rok = (h > 0 ? 1u : 0u) | 2u | (h + 1 < (uint32_t)a.H ? 4u : 0u);
      const uint32_t cok = (w > 0 ? 1u : 0u) | 2u | (w + 1 < (uint32_t)a.W ? 4u : 0u);
      // tap = 3*(dr+1) + (ds+1): mask = rows (x) cols outer product
      uint32_t msk = 0;
      msk |= (rok & 1u) ? cok : 0u;
      msk |= (rok & 2u) ? (cok << 3) : 0u;
      msk |= (rok & 4u) ? (cok << 6) : 0u;
      if (a.taps == 1) msk = 1u;
      nmask[r] = valid ? ~msk : ~0u;
      pb1[r] = (mm * (uint32_t)a.pitch1 + (uint32_t)gch * 8u) * 2u;
      pb2[r] = (mm * (uint32_t)a.pitch2 + (uint32_t)gch * 8u) * 2u;
    }
#pragma unroll
    for (int f = 0; f < WPIECES; ++f) {
      const int n = tn * BN + (wave * WPIECES + f) * 8 + (lane >> 3);
      woff[f] = (uint32_t)(n * a.ldw + gch * 8) * 2u;
    }
  };

  auto issue = [&](int ks, char* buf) {
    if (a.packed) {
      const int tap = ks * 8 + gch;  // per lane; taps >= 9 have no mask bit -> zeros
      const int toff = (tap_dr(tap) * a.W + tap_ds(tap)) * a.pitch1 * 2 - gch * 16;
#pragma unroll
      for (int r = 0; r < NROW; ++r) {
        const uint32_t bad = tap < 9 ? (nmask[r] >> tap) & 1u : 1u;
        const uint32_t off = (bad << 31) | (uint32_t)((int)pb1[r] + toff);
        dma16(rx1, (lds_void*)(buf + (wave * NROW + r) * 1024), off);
      }
    } else {
      const int c0 = icc * 64;
      const bool s2 = c0 >= a.C1;
      const int pitch = s2 ? a.pitch2 : a.pitch1;
      const int tap_lin = a.taps == 9 ? tap_dr(itap) * a.W + tap_ds(itap) : 0;
      const int soff = (tap_lin * pitch + (s2 ? c0 - a.C1 : c0)) * 2;  // wave-uniform (SGPR)
      const int bit = a.taps == 9 ? itap : 0;
#pragma unroll
      for (int r = 0; r < NROW; ++r) {
        const uint32_t bad = __builtin_amdgcn_ubfe(nmask[r], (uint32_t)bit, 1u);
        const uint32_t off = (bad << 31) | (uint32_t)((int)(s2 ? pb2[r] : pb1[r]) + soff);
        dma16(s2 ? rx2 : rx1, (lds_void*)(buf + (wave * NROW + r) * 1024), off);
      }
      if (++icc == a.cpt) { icc = 0; ++itap; if (itap == a.taps) itap = 0; }
    }
    char* wbuf = buf + P_BYTES;
#pragma unroll
    for (int f = 0; f < WPIECES; ++f)
      dma16(rw, (lds_void*)(wbuf + (wave * WPIECES + f) * 1024), woff[f] + (uint32_t)(ks0 + ks) * 128u);
  };

  // LDS byte offsets of this lane's fragment reads (k-half hf) relative to a 16-row subtile
  int rdoff[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) rdoff[hf] = (lane & 15) * 128 + 16 * (((lane >> 4) + 4 * hf) ^ (lane & 7));

  const auto ry1 = make_rsrc(a.y1, a.ybytes1);
  const auto ry2 = make_rsrc(a.y2 ? a.y2 : a.y1, a.y2 ? a.ybytes2 : 0u);

  f32x4 acc[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  int ks = 0, t = 0;    // compute position (K step within tile, tile index)
  int iks = 0, it = 0;  // issue position (K step within tile, tile index) of the newest stage
  int ig = 0;           // global index of the newest issued stage
  int ibuf = 0, cbuf = 0;  // LDS buffer of the newest issued stage / of the stage being computed
  if (total > 0) {
    set_tile(0);
    issue(0, smem);
  }
  // vector-memory stores the previous step's epilogue issued after stage g's DMA: vmcnt counts
  // them in issue order, so stage g has landed once at most that many ops are outstanding (a plain
  // vmcnt(0) would also wait for the output stores of every tile before its next K step)
  int pend = 0;
  // Training BN statistics accumulate over ALL of this block's tiles: with the persistent grid a
  // multiple of tilesN (host-checked), block lid always has channel tile tn = lid % tilesN, so one
  // slab row per (lid / tilesN, wm) -- grid * WAVES_M / tilesN rows instead of one per M-tile
  // (65536 at 256^2 x 64 ch, bs 64), written once after the last tile.
  float s1[NJ][4], s2[NJ][4];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[j][r] = 0.f; s2[j][r] = 0.f; }
  for (int g = 0; g < total; ++g) {
    // stage g has landed once at most (epilogue stores issued after it) ops are outstanding
    // (in-order completion); older stores are not counted, which only makes the wait stricter
    vm_wait_p<0, 2 * NJ, 4 * NJ>(pend);
    pend = 0;
    raw_barrier();
    if (ig + 1 < total) {  // the buffer computed at step g-1: every wave is past it (barrier above)
      if (++iks == a.nks) { iks = 0; ++it; set_tile(it); }
      ibuf = ibuf + 1 == NST ? 0 : ibuf + 1;
      issue(iks, smem + ibuf * BUF);
      ++ig;
    }
    const char* pb = smem + cbuf * BUF;
    cbuf = cbuf + 1 == NST ? 0 : cbuf + 1;
    const char* wb = pb + P_BYTES;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      bf16x8 fa[NJ], fb[4];
#pragma unroll
      for (int j = 0; j < NJ; ++j) fa[j] = *(const bf16x8*)(wb + (wn * NJ + j) * 2048 + rdoff[hf]);
#pragma unroll
      for (int i = 0; i < 4; ++i) fb[i] = *(const bf16x8*)(pb + (wm * 4 + i) * 2048 + rdoff[hf]);
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[j], fb[i], acc[j][i], 0, 0, 0);
    }
    if (++ks < a.nks) continue;

    // ---- epilogue of tile t: acc[j][i][r] = out[m = m0 + wm*64 + 16i + (lane&15)][n = n0 + wn*64 + 16j + 4*(lane>>4) + r]
    ks = 0;
    const int item = (int)lid + t * (int)G;
    ++t;
    int tile = item;
    if (a.ksplit > 1) {  // fp32 partial tile -> slab[split][m][n]
      const int tiles1 = a.ntiles / a.ksplit;
      tile = item % tiles1;
      const int split = item / tiles1;
      const int tm = tile / a.tilesN, tn = tile - tm * a.tilesN;
      const auto rk = make_rsrc(a.kslab, (uint32_t)((long)a.ksplit * a.M * a.Cout * 4));
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = tn * BN + wn * WNT + j * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = tm * BM + wm * 64 + i * 16 + (lane & 15);
          const f32x4 o = acc[j][i];
          acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
          const uint32_t off = m < a.M ? (uint32_t)(((long)split * a.M + m) * a.Cout + n) * 4u : RDP_OOB;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rk, off, 0, 0);
        }
      }
      pend = 4 * NJ;  // NJ x 4 slab stores; the epilogue runs in conv_splitk_reduce_kernel
      continue;
    }
    const int tm = tile / a.tilesN, tn = tile - tm * a.tilesN;
    const int m0 = tm * BM, n0 = tn * BN;
    // Widened stores: a lane holds 4 couts (16 j + 4 g + r, g = lane >> 4) of one pixel per
    // fragment. v_permlane16_swap of fragment pair (j, j+1) gives every lane 8 consecutive couts
    // (lanes g: 0 -> 0..7, 1 -> 16..23, 2 -> 8..15, 3 -> 24..31 of the pair) = one 16-B store, and a
    // pixel's 32 couts become 64 contiguous bytes per instruction (cdna_hip_programming.md T21).
    const int gq = lane >> 4;
    const int coff = 16 * (gq & 1) + 8 * (gq >> 1);
#pragma unroll
    for (int jp = 0; jp < NJ; jp += 2) {
      const int nb = n0 + wn * WNT + jp * 16;  // first cout of the pair
      const int n = nb + coff;                  // this lane's 8 couts after the swap
      const bool d2 = n >= a.Cy1;
      const int nn = d2 ? n - a.Cy1 : n;
      const int yp = d2 ? a.ypitch2 : a.ypitch1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + (lane & 15);
        uint2 v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int j = jp + h;
          f32x4 o = acc[j][i];
          if (a.escale) {
            const int nc = nb + h * 16 + 4 * gq;
            const float4 sc = *(const float4*)(a.escale + nc), sh = *(const float4*)(a.eshift + nc);
            o[0] = fmaf(o[0], sc.x, sh.x); o[1] = fmaf(o[1], sc.y, sh.y);
            o[2] = fmaf(o[2], sc.z, sh.z); o[3] = fmaf(o[3], sc.w, sh.w);
            if (a.erelu) {
              o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f); o[2] = fmaxf(o[2], 0.f); o[3] = fmaxf(o[3], 0.f);
            }
          }
          v[h].x = pack2bf(o[0], o[1]);
          v[h].y = pack2bf(o[2], o[3]);
          acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (a.stats) {
            bn_stats4(v[h], s1[j], s2[j]);
          }
        }
        const auto rxs = __builtin_amdgcn_permlane16_swap(v[0].x, v[1].x, false, false);
        const auto rys = __builtin_amdgcn_permlane16_swap(v[0].y, v[1].y, false, false);
        const uint32_t off = m < a.M ? (uint32_t)(m * yp + nn) * 2u : RDP_OOB;
        bstore16(d2 ? ry2 : ry1, off, make_uint4(rxs[0], rys[0], rxs[1], rys[1]));
      }
    }
    pend = 2 * NJ;  // 2 NJ output stores
  }
  if (a.stats && a.ksplit == 1 && total > 0) {
    // reduce over the 16 pixel lanes (lane & 15) sharing a channel group; one slab row per (block group, wm)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s1[j][r] = row16_sum(s1[j][r]);
        s2[j][r] = row16_sum(s2[j][r]);
      }
    if ((lane & 15) == 0) {
      const int tn = (int)lid % a.tilesN;
      float* row = a.stats + (size_t)(((int)lid / a.tilesN) * WAVES_M + wm) * 2 * a.Cout;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = tn * BN + wn * WNT + j * 16 + 4 * (lane >> 4);
        *(float4*)(row + c) = make_float4(s1[j][0], s1[j][1], s1[j][2], s1[j][3]);
        *(float4*)(row + a.Cout + c) = make_float4(s2[j][0], s2[j][1], s2[j][2], s2[j][3]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Ping-pong 256 x BN tile (BN = 256 or 128): 8 waves, ONE block per CU, 2-3 stage K ring.
//
// The 2-barrier structure above (2 blocks / CU, 128 x 128 tiles) tops out near 0.9-1.1 PF: every
// K step waits for its own stage behind one barrier, with about one K step of MFMA work to hide
// the DMA. Here the two wave groups of the block (wm = 0: waves 0-3, wm = 1: waves 4-7; one wave
// of each group per SIMD) run staggered by one barrier (cdna_hip_programming.md "The 256^2 8-phase
// template", T3+T4+T5): while one group issues its LDS fragment reads and DMA, its partner on the
// same SIMD runs a 16-MFMA cluster. A K step (64 channels of one tap) is NPH phases; a phase is a
// memory segment (fragment reads [+ the DMA of a later stage at phase 0] + lgkmcnt(0)) and a
// compute segment (16 MFMAs), each ended by one raw s_barrier. Stage g+NST-1 is issued at phase 0
// of K step g and waited for (counted vmcnt, never a drain of newer stages) in the memory segment
// of the last phase of K step NST-2 later, i.e. 1.5 K steps (NST 2) to 2.5 K steps (NST 3) of
// MFMA work hide each DMA -- and the 256-wide tile halves the LDS fill bytes per FLOP of the
// 128 x 128 tile. Ordering (one barrier more than unstaggered, as the template requires):
//   * RAW: each wave waits for its own DMA of stage g+1 in M(g, NPH-1); group 1 runs that segment
//     one slot later than group 0, i.e. in the slot just before group 0's first read M(g+1, 0).
//   * WAR: every memory segment ends with lgkmcnt(0), so the last reads of a buffer (M(g-1,
//     NPH-1), group 1 one slot later) are complete before the barrier that precedes the first DMA
//     into it (M(g, 0) of group 0).
// Accumulation order per output element is the K-step order with the two K halves of a step in
// order, exactly as conv_igemm_kernel: outputs are bitwise equal to it. Training BN statistics
// accumulate per block in LDS words owned by one lane each (no registers held across tiles).
// Generic (non-packed) im2col only, no split-K / fused pool or upsample.
// Fragment reads of phases 0..NPH-2 stay in flight across the segment barrier; at BN = 256 both
// cout halves of the weight fragments stay in registers (HOLDB: no re-read in phase 3); BN = 128
// runs a 3-stage K ring (NST). (A 512 x 64 form and a BN-backward reduction in the dgrad epilogue
// were measured slower: profiles/dead_ends.md.)
// UT: ConvTranspose2d sub-pixel output (ConvArgs tlc / ubias; no stats, no split); UTR: the
// ConvTranspose2d input gradient, the A operand read at the 4 sub-pixels of the output gradient
// (taps = 4, ConvArgs tH2 / tW2 / toy / tox) -- their own instantiations, so the plain kernels'
// scalar registers are untouched.
template <int BN, bool SPLIT = false, bool UT = false, bool UTR = false>
__global__ __launch_bounds__(512, 1) void conv_pp_kernel(const ConvArgs a) {
  // 256-pixel tile, wave (wm, wn) = 128 pixels x BN/4 couts
  constexpr int NST = BN == 128 ? 3 : 2;
  constexpr bool RD_INFLIGHT = true, HOLDB = BN == 256;
  constexpr int BM = 256;
  constexpr int WNT = BN / 4;        // couts per wave
  constexpr int NJ = WNT / 16;       // cout fragments per wave (4 / 2)
  constexpr int NI = 8;              // pixel fragments per wave
  constexpr int NPH = (NJ / 2) * (NI / 4);  // phases per K step, 16 MFMAs each (4 / 2)
  constexpr int P_BYTES = BM * 128, W_BYTES = BN * 128, BUF = P_BYTES + W_BYTES;
  constexpr int NROW = BM / 64;      // 8-row pixel DMA pieces per wave per stage
  constexpr int WPIECES = BN / 64;   // weight DMA pieces per wave per stage
  constexpr int DMA_OPS = NROW + WPIECES;
  constexpr int SROWS = 2;           // statistics rows per block (one per wave row)
  constexpr int ST_OFF = NST * BUF;   // BN statistics: [SROWS][2][BN] fp32
  static_assert(NST * BUF + SROWS * 2 * BN * 4 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[NST * BUF + SROWS * 2 * BN * 4];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int gch = (lane & 7) ^ (lane >> 3);
  const int wpx = wm * 128;   // first pixel row of this wave in the tile
  const int wco = wn * WNT;   // first cout of this wave in the tile

  const uint32_t G = gridDim.x;
  const uint32_t lid = xcd_remap(blockIdx.x, G);
  const int my_tiles = lid < (uint32_t)a.ntiles ? (a.ntiles - 1 - (int)lid) / (int)G + 1 : 0;
  const int total = my_tiles * a.nks;

  const auto rx1 = make_rsrc(a.x1, a.xbytes1);
  const auto rx2 = make_rsrc(a.x2 ? a.x2 : a.x1, a.x2 ? a.xbytes2 : 0u);
  const auto rw = make_rsrc(a.w, a.wbytes);
  const auto ry1 = make_rsrc(a.y1, a.ybytes1);
  const auto ry2 = make_rsrc(a.y2 ? a.y2 : a.y1, a.y2 ? a.ybytes2 : 0u);

  // DMA state of the tile being staged (see conv_igemm_kernel::set_tile). Split-K (ksplit > 1):
  // work item = (tile, split) as in conv_igemm_kernel, K steps [ks0, ks0 + nks) of the tile.
  const int tiles1 = SPLIT ? a.ntiles / a.ksplit : a.ntiles;
  uint32_t pb1[NROW], pb2[NROW], nmask[NROW], woff[WPIECES];
  int itap = 0, icc = 0;
  auto set_tile = [&](int t) {
    const int item = (int)lid + t * (int)G;
    const int tile = SPLIT ? item % tiles1 : item;
    const int ks0 = SPLIT ? (item / tiles1) * a.nks : 0;
    itap = ks0 / a.cpt;
    icc = ks0 - itap * a.cpt;
    const int tm = tile / a.tilesN, tn = tile - tm * a.tilesN;
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
      const int m = tm * BM + (wave * NROW + r) * 8 + (lane >> 3);
      const bool valid = m < a.M;
      const uint32_t mm = valid ? (uint32_t)m : 0u;
      const uint32_t img = (__umulhi(mm, a.fhw_m) + mm) >> a.fhw_s;
      const uint32_t hw = mm - img * (uint32_t)(a.H * a.W);
      const uint32_t h = (__umulhi(hw, a.fw_m) + hw) >> a.fw_s;
      const uint32_t w = hw - h * (uint32_t)a.W;
      if constexpr (UTR) {  // the (2h + toy, 2w + tox) pixel of the output-gradient map; 4 valid taps
        const uint32_t px = (img * (uint32_t)a.tH2 + 2u * h + (uint32_t)a.toy) * (uint32_t)a.tW2 + 2u * w + (uint32_t)a.tox;
        nmask[r] = valid ? ~0xfu : ~0u;
        pb1[r] = (px * (uint32_t)a.pitch1 + (uint32_t)gch * 8u) * 2u;
        pb2[r] = pb1[r];
        continue;
      }
      const uint32_t rok = (h > 0 ? 1u : 0u) | 2u | (h + 1 < (uint32_t)a.H ? 4u : 0u);
      const uint32_t cok = (w > 0 ? 1u : 0u) | 2u | (w + 1 < (uint32_t)a.W ? 4u : 0u);
      uint32_t msk = 0;
      msk |= (rok & 1u) ? cok : 0u;
      msk |= (rok & 2u) ? (cok << 3) : 0u;
      msk |= (rok & 4u) ? (cok << 6) : 0u;
      if (a.taps == 1) msk = 1u;
      nmask[r] = valid ? ~msk : ~0u;
      pb1[r] = (mm * (uint32_t)a.pitch1 + (uint32_t)gch * 8u) * 2u;
      pb2[r] = (mm * (uint32_t)a.pitch2 + (uint32_t)gch * 8u) * 2u;
    }
#pragma unroll
    for (int f = 0; f < WPIECES; ++f) {
      const int n = tn * BN + (wave * WPIECES + f) * 8 + (lane >> 3);
      woff[f] = (uint32_t)(n * a.ldw + gch * 8 + ks0 * 64) * 2u;  // + the split's first K column
    }
  };
  auto issue = [&](int ks, char* buf) {
    const int c0 = icc * 64;
    const bool s2 = c0 >= a.C1;
    const int pitch = s2 ? a.pitch2 : a.pitch1;
    const int tap_lin = UTR ? (itap >> 1) * a.tW2 + (itap & 1) : a.taps == 9 ? tap_dr(itap) * a.W + tap_ds(itap) : 0;
    const int soff = (tap_lin * pitch + (s2 ? c0 - a.C1 : c0)) * 2;
    const int bit = UTR || a.taps == 9 ? itap : 0;
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
      const uint32_t bad = __builtin_amdgcn_ubfe(nmask[r], (uint32_t)bit, 1u);
      const uint32_t off = (bad << 31) | (uint32_t)((int)(s2 ? pb2[r] : pb1[r]) + soff);
      dma16(s2 ? rx2 : rx1, (lds_void*)(buf + (wave * NROW + r) * 1024), off);
    }
    if (++icc == a.cpt) { icc = 0; ++itap; if (itap == a.taps) itap = 0; }
    char* wbuf = buf + P_BYTES;
#pragma unroll
    for (int f = 0; f < WPIECES; ++f)
      dma16(rw, (lds_void*)(wbuf + (wave * WPIECES + f) * 1024), woff[f] + (uint32_t)ks * 128u);
  };

  int rdoff[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) rdoff[hf] = (lane & 15) * 128 + 16 * (((lane >> 4) + 4 * hf) ^ (lane & 7));

  const int srow = wm;
  float* const sst = (float*)(smem + ST_OFF) + srow * 2 * BN;  // this wave (row)'s statistics words
  // UT: the bias in the (unused) statistics words, read by the epilogue with LDS loads -- a global load
  // there would wait (vmcnt) for the in-flight DMA stages too. 2^tlc <= 4 BN floats (host-checked).
  const float* const sbias = (const float*)(smem + ST_OFF);
  if constexpr (UT) {
    for (int c = (int)threadIdx.x * 4; c < (1 << a.tlc); c += 512 * 4)
      *(float4*)(smem + ST_OFF + c * 4) = *(const float4*)(a.ubias + c);
  }
  if (a.stats && (lane & 15) == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = wco + j * 16 + 4 * (lane >> 4);
      *(float4*)(sst + c) = make_float4(0.f, 0.f, 0.f, 0.f);
      *(float4*)(sst + BN + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  f32x4 acc[NJ][NI];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // [cout half held][k half][cout frag of the phase] / [k half][pixel frag of the phase]
  bf16x8 fa[HOLDB ? 2 : 1][2][2], fb[2][4];

  int ks = 0, t = 0;              // compute position
  int iks = 0, it = 0, ig = 0;    // newest issued stage: K step, tile, global index
  int cbuf = 0, ibuf = 0;
  if (total > 0) {
    set_tile(0);
    issue(0, smem);
    if (NST > 2 && total > 1) {
      if (++iks == a.nks) { iks = 0; ++it; set_tile(it); }
      issue(iks, smem + BUF);
      ig = 1;
      ibuf = 1;
    }
    if (ig > 0) vm_wait<DMA_OPS>();
    else vm_wait<0>();
  }
  raw_barrier();
  if (wm == 1) raw_barrier();  // stagger the two wave groups by one segment

  auto epilogue = [&]() {
    const int item = (int)lid + t * (int)G;
    if constexpr (SPLIT) {  // fp32 partial tile -> slab[split][m][n]; conv_splitk_reduce_kernel finishes
      const int tile = item % tiles1, split = item / tiles1;
      const int tm = tile / a.tilesN, tn = tile - tm * a.tilesN;
      const auto rk = make_rsrc(a.kslab, (uint32_t)((long)a.ksplit * a.M * a.Cout * 4));
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = tn * BN + wco + j * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int m = tm * BM + wpx + i * 16 + (lane & 15);
          const uint32_t off = m < a.M ? (uint32_t)(((long)split * a.M + m) * a.Cout + n) * 4u : RDP_OOB;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[j][i]), rk, off, 0, 0);
          acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      return;
    }
    const int tm = item / a.tilesN, tn = item - tm * a.tilesN;
    const int m0 = tm * BM, n0 = tn * BN;
    const int gq = lane >> 4;
    const int coff = 16 * (gq & 1) + 8 * (gq >> 1);
    float s1[NJ][4], s2[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) { s1[j][r] = 0.f; s2[j][r] = 0.f; }
#pragma unroll
    for (int jp = 0; jp < NJ; jp += 2) {
      const int nb = n0 + wco + jp * 16;
      const int n = nb + coff;
      const bool d2 = nb >= a.Cy1;  // wave-uniform: Cy1 % 32 == 0 (host-checked), one SRD per store
      const int nn = d2 ? n - a.Cy1 : n;
      const int yp = d2 ? a.ypitch2 : a.ypitch1;
      // UT: sub-pixel of this cout pair (wave-uniform: 2^tlc >= 64) and its offset from the (2h, 2w) pixel
      const int sub = UT ? nb >> a.tlc : 0, cmask = UT ? (1 << a.tlc) - 1 : 0;
      const int subo = UT ? ((sub >> 1) * a.tW2 + (sub & 1)) * yp + (n & cmask) : 0;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int m = m0 + wpx + i * 16 + (lane & 15);
        uint2 v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int j = jp + h;
          f32x4 o = acc[j][i];
          if (a.escale) {
            const int nc = nb + h * 16 + 4 * gq;
            const float4 sc = *(const float4*)(a.escale + nc), sh = *(const float4*)(a.eshift + nc);
            o[0] = fmaf(o[0], sc.x, sh.x); o[1] = fmaf(o[1], sc.y, sh.y);
            o[2] = fmaf(o[2], sc.z, sh.z); o[3] = fmaf(o[3], sc.w, sh.w);
            if (a.erelu) {
              o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f); o[2] = fmaxf(o[2], 0.f); o[3] = fmaxf(o[3], 0.f);
            }
          } else if (UT) {
            const float4 b = *(const float4*)(sbias + ((nb + h * 16 + 4 * gq) & cmask));
            o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
          }
          v[h].x = pack2bf(o[0], o[1]);
          v[h].y = pack2bf(o[2], o[3]);
          acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (a.stats && m < a.M) {
            bn_stats4(v[h], s1[j], s2[j]);
          }
        }
        const auto rxs = __builtin_amdgcn_permlane16_swap(v[0].x, v[1].x, false, false);
        const auto rys = __builtin_amdgcn_permlane16_swap(v[0].y, v[1].y, false, false);
        uint32_t pix = (uint32_t)m * (uint32_t)yp + (uint32_t)nn;
        if constexpr (UT) {  // low-res pixel (img, h, w) -> the (2h + toy, 2w + tox) pixel of the output map
          // W % 16 == 0: the 16 pixels of fragment row i lie in one image row, so the division runs once
          // on the (wave-uniform) first pixel; else per lane
          const bool row16 = (a.W & 15) == 0;
          const uint32_t mm = row16 ? (uint32_t)(m0 + wpx + i * 16) : (uint32_t)m;
          const uint32_t img = fdiv(mm, a.fhw_m, a.fhw_s);
          const uint32_t hw = mm - img * (uint32_t)(a.H * a.W);
          const uint32_t hh = fdiv(hw, a.fw_m, a.fw_s);
          const uint32_t ww = hw - hh * (uint32_t)a.W + (row16 ? (uint32_t)(lane & 15) : 0u);
          pix = ((img * (uint32_t)a.tH2 + 2u * hh + (uint32_t)a.toy) * (uint32_t)a.tW2 + 2u * ww + (uint32_t)a.tox) *
                    (uint32_t)yp + (uint32_t)subo;
        }
        const uint32_t off = m < a.M ? pix * 2u : RDP_OOB;
        bstore16(d2 ? ry2 : ry1, off, make_uint4(rxs[0], rys[0], rxs[1], rys[1]));
      }
    }
    if (a.stats) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s1[j][r] = row16_sum(s1[j][r]);
          s2[j][r] = row16_sum(s2[j][r]);
        }
      if ((lane & 15) == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int c = wco + j * 16 + 4 * gq;
          float4 u = *(float4*)(sst + c), q = *(float4*)(sst + BN + c);
          u.x += s1[j][0]; u.y += s1[j][1]; u.z += s1[j][2]; u.w += s1[j][3];
          q.x += s2[j][0]; q.y += s2[j][1]; q.z += s2[j][2]; q.w += s2[j][3];
          *(float4*)(sst + c) = u;
          *(float4*)(sst + BN + c) = q;
        }
      }
    }
  };

  for (int g = 0; g < total; ++g) {
    const char* pb = smem + cbuf * BUF;
    const char* wb = pb + P_BYTES;
#pragma unroll
    for (int p = 0; p < NPH; ++p) {
      // phase -> (pixel half ih, cout half jh): BN 256: (0,0) (0,1) (1,1) (1,0); BN 128: (0,*) (1,*)
      const int ih = NPH == 4 ? (p >> 1) : p;
      const int jh = NPH == 4 ? (((p + 1) >> 1) & 1) : 0;
      const bool new_b = NPH == 4 ? (p == 0 || p == 2) : true;
      const bool new_a = NPH == 4 ? (HOLDB ? p < 2 : p != 2) : (p == 0);
      const int fh = HOLDB ? jh : 0;  // register set of the phase's weight fragments
      // ---- memory segment
      if (p == 0 && ig + 1 < total) {
        if (++iks == a.nks) { iks = 0; ++it; set_tile(it); }
        ibuf = ibuf + 1 == NST ? 0 : ibuf + 1;
        issue(iks, smem + ibuf * BUF);
        ++ig;
      }
      if (new_a) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int j = 0; j < 2; ++j) fa[fh][hf][j] = *(const bf16x8*)(wb + (wco / 16 + jh * 2 + j) * 2048 + rdoff[hf]);
      }
      if (new_b) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
          for (int i = 0; i < 4; ++i) fb[hf][i] = *(const bf16x8*)(pb + (wpx / 16 + ih * 4 + i) * 2048 + rdoff[hf]);
      }
      // The last memory segment of a K step drains its fragment reads (lgkmcnt(0)) before the barrier:
      // the next DMA into this buffer follows that barrier (WAR). The other phases' reads stay in
      // flight across the barrier and are waited for by the MFMAs that use them (the segment ends as
      // soon as they are issued; their LDS latency overlaps the partner group's MFMA cluster).
      if (p == NPH - 1 && g + 1 < total) {  // + this wave's DMA of stage g+1 has landed
        if (ig > g + 1) vm_wait<DMA_OPS>();
        else vm_wait<0>();
      } else if (p == NPH - 1 || !RD_INFLIGHT) {
        wait_lgkm0();
      }
      raw_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- compute segment
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[jh * 2 + j][ih * 4 + i] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[fh][hf][j], fb[hf][i], acc[jh * 2 + j][ih * 4 + i], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      if (p == NPH - 1 && ks + 1 == a.nks) epilogue();
      __builtin_amdgcn_sched_barrier(0);
      raw_barrier();
    }
    cbuf = cbuf + 1 == NST ? 0 : cbuf + 1;
    if (++ks == a.nks) { ks = 0; ++t; }
  }
  if (wm == 0) raw_barrier();  // same barrier count for both groups
  if (a.stats && total > 0 && (lane & 15) == 0) {
    const int tn = (int)lid % a.tilesN;
    float* row = a.stats + (size_t)(((int)lid / a.tilesN) * SROWS + srow) * 2 * a.Cout;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cl = wco + j * 16 + 4 * (lane >> 4);
      *(float4*)(row + tn * BN + cl) = *(const float4*)(sst + cl);
      *(float4*)(row + a.Cout + tn * BN + cl) = *(const float4*)(sst + BN + cl);
    }
  }
}

// what the plan's geometry functions (conv_plan.h) see of a filled ConvArgs
static RdpGemmShape gemm_shape(const ConvArgs& a) {
  RdpGemmShape g;
  g.M = a.M; g.Cout = a.Cout; g.Cy1 = a.Cy1; g.nks = a.nks; g.packed = a.packed; g.stats = a.stats != nullptr;
  g.N = a.N; g.uH = a.up ? a.uH : 0;
  return g;
}
static RdpConvFuseOk fuse_of(const ConvArgs& a) { return {a.pool != nullptr, a.up != nullptr, a.bnpart != nullptr}; }

static int launch_split_reduce(const ConvArgs& a, const RdpIgemmGeo& g, hipStream_t s, int* pooled);

// ksplit > 1 (rdp_pp_split's d, a.kslab set): fp32 partial tiles, then the shared split-K reduce (stats / eval
// epilogue / fused pool or upsample).
template <int BN>
static int launch_pp(ConvArgs a, hipStream_t s, int ksplit = 1, int* pooled = nullptr) {
  const RdpIgemmGeo g = rdp_pp_geo(gemm_shape(a), BN, ksplit, a.kslab != nullptr, fuse_of(a));
  if (!g.fits) return -1;
  a.tilesN = g.tilesN; a.ntiles = g.ntiles; a.ksplit = g.ksplit; a.nks = g.nks;
  if (g.ksplit > 1) {
    ConvArgs k = a;
    k.stats = nullptr;  // statistics come from the reduce
    hipLaunchKernelGGL((conv_pp_kernel<BN, true>), dim3(g.grid), dim3(512), 0, s, k);
    return launch_split_reduce(a, g, s, pooled);
  }
  a.pool = nullptr;
  a.up = nullptr;
  if (a.tlc || a.taps == 4) {  // ConvTranspose2d output (rdp_conv_upT_fwd) / input gradient (rdp_conv_upT_dgrad)
    if (a.stats || a.escale || a.y2) return -1;
    if (a.tlc) hipLaunchKernelGGL((conv_pp_kernel<BN, false, true>), dim3(g.grid), dim3(512), 0, s, a);
    else hipLaunchKernelGGL((conv_pp_kernel<BN, false, false, true>), dim3(g.grid), dim3(512), 0, s, a);
    return 0;
  }
  hipLaunchKernelGGL((conv_pp_kernel<BN>), dim3(g.grid), dim3(512), 0, s, a);
  return g.rows;
}

static ConvArgs conv_args(const RdpConv& c, int taps, int packed, float* ws, const RdpConvFuse& fuse, int* pooled,
                          const RdpConvBnBwd& bn, int* bnrows);

// ConvArgs of a ConvTranspose2d launch: one source, one destination of all Cout GEMM columns, the placement
static ConvArgs upT_args(const RdpConv& c, int taps, const RdpUpT& t) {
  ConvArgs a = conv_args(c, taps, 0, nullptr, RdpConvFuse{}, nullptr, RdpConvBnBwd{}, nullptr);
  a.pitch2 = a.pitch1; a.ypitch2 = a.ypitch1; a.Cy1 = a.Cout;
  a.tH2 = t.H2; a.tW2 = t.W2; a.toy = t.oy; a.tox = t.ox;
  return a;
}

int rdp_conv_upT_fwd(const RdpConv& c, const RdpUpT& t, const float* bias, hipStream_t s) {
  const RdpUpTGeo g = rdp_upT_fwd_geo(c, t);
  if (!g.fits) return -1;
  ConvArgs a = upT_args(c, 1, t);
  a.ubias = bias;
  a.tlc = g.tlc;
  return (g.BN == 256 ? launch_pp<256>(a, s) : launch_pp<128>(a, s)) >= 0 ? 0 : -1;
}

int rdp_conv_upT_dgrad(const RdpConv& c, const RdpUpT& t, hipStream_t s) {
  const RdpUpTGeo g = rdp_upT_dgrad_geo(c, t);
  if (!g.fits) return -1;
  const ConvArgs a = upT_args(c, 4, t);
  return (g.BN == 256 ? launch_pp<256>(a, s) : launch_pp<128>(a, s)) >= 0 ? 0 : -1;
}



// Split-K reduction + epilogue: y[m][n] = epi(sum_s slab[s][m][n]); optional BN-stats rows (one per
// block). Thread = fixed 4-channel group (epilogue coefficients in registers), rows grid-strided.
// The slices are read 8 at a time as independent 16-B buffer loads (slices past ksplit read zeros
// from an out-of-range offset: no branch around the loads) into 4 accumulators summed in a fixed
// order: a dependent load per slice made this kernel one L2 round trip per slice (7-8 us at 18
// slices at N = 1; the serving convs reduce 2-18 slices).
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvArgs a, int nrow_blocks) {
  extern __shared__ float sst[];  // [rows][2][Cout] stats staging
  const int CG = a.Cout >> 2, RPB = 256 / CG;  // Cout power of two, 64 <= Cout <= 1024
  const int g = threadIdx.x & (CG - 1), r = threadIdx.x / CG;
  const int n = g * 4;
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.escale) sc = *(const float4*)(a.escale + n);
  if (a.eshift) sh = *(const float4*)(a.eshift + n);
  const bool d2 = n >= a.Cy1;
  const int nn = d2 ? n - a.Cy1 : n;
  u16* const y = d2 ? a.y2 : a.y1;
  const int yp = d2 ? a.ypitch2 : a.ypitch1;
  const auto rk = make_rsrc(a.kslab, (uint32_t)((long)a.ksplit * a.M * a.Cout * 4));
  const uint32_t sstride = (uint32_t)a.M * (uint32_t)a.Cout * 4u;  // bytes between slices
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  // sum of the slices + epilogue for pixel m -> 4 bf16 (packed), stored to y
  auto pixel = [&](int m) -> uint2 {
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t base = ((uint32_t)m * (uint32_t)a.Cout + (uint32_t)n) * 4u;
    for (int sp0 = 0; sp0 < a.ksplit; sp0 += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t off = sp0 + u < a.ksplit ? base + (uint32_t)(sp0 + u) * sstride : RDP_OOB;
        v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u & 3] += v[u];
    }
    f32x4 o = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    o[0] = fmaf(o[0], sc.x, sh.x); o[1] = fmaf(o[1], sc.y, sh.y);
    o[2] = fmaf(o[2], sc.z, sh.z); o[3] = fmaf(o[3], sc.w, sh.w);
    if (a.erelu) {
      o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f); o[2] = fmaxf(o[2], 0.f); o[3] = fmaxf(o[3], 0.f);
    }
    const uint2 w = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
    *(uint2*)(y + (long)m * yp + nn) = w;
    return w;
  };
  if (a.pool) {
    // eval-mode MaxPool2d(2) of the output, fused: a thread owns 2x2 windows (H, W even)
    const int Ho = a.H >> 1, Wo = a.W >> 1, nwin = a.M >> 2;
    for (int wi = blockIdx.x * RPB + r; wi < nwin; wi += nrow_blocks * RPB) {
      const int img = wi / (Ho * Wo), rem = wi - img * (Ho * Wo), ho = rem / Wo, wo = rem - ho * Wo;
      const int m00 = (img * a.H + 2 * ho) * a.W + 2 * wo;
      const uint2 q[4] = {pixel(m00), pixel(m00 + 1), pixel(m00 + a.W), pixel(m00 + a.W + 1)};
      float mx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t wd = k < 2 ? q[0].x : q[0].y;
        mx[k] = (k & 1) ? bfhi(wd) : bflo(wd);
      }
#pragma unroll
      for (int t = 1; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t wd = k < 2 ? q[t].x : q[t].y;
          mx[k] = fmaxf(mx[k], (k & 1) ? bfhi(wd) : bflo(wd));
        }
      *(uint2*)(a.pool + (long)wi * a.ppitch + n) = make_uint2(pack2bf(mx[0], mx[1]), pack2bf(mx[2], mx[3]));
    }
    return;  // eval: no statistics
  }
  // BN-backward partials (a.bnpart): the owner layer's coefficients of this thread's 4 channels
  const bool bnr = a.stats == nullptr && a.bnpart != nullptr;
  float bmean[4], binv[4], bsc[4], bsh[4];
  if (bnr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      bmean[k] = a.bncoef[bn_off(BN_MEAN, a.Cout) + n + k];
      binv[k] = a.bncoef[bn_off(BN_INVSTD, a.Cout) + n + k];
      bsc[k] = a.bncoef[bn_off(BN_SCALE, a.Cout) + n + k];
      bsh[k] = a.bncoef[bn_off(BN_SHIFT, a.Cout) + n + k];
    }
  }
  for (int m = blockIdx.x * RPB + r; m < a.M; m += nrow_blocks * RPB) {
    const uint2 w = pixel(m);
    if (a.stats) {
      bn_stats4(w, s1, s2);
    } else if (bnr) {  // w = dL/da (as stored, bf16) of the owner's post-ReLU activation
      float q[4], fy[4];
      unpack4(w, q);
      unpack4(*(const uint2*)(a.bny + (long)m * a.bnypitch + n), fy);
      bn_acc_n(q, fy, bmean, binv, bsc, bsh, s1, s2);
    }
  }
  float* const rows_out = a.stats ? a.stats : (bnr ? a.bnpart : nullptr);
  if (!rows_out) return;
  *(float4*)(sst + (r * 2 + 0) * a.Cout + n) = make_float4(s1[0], s1[1], s1[2], s1[3]);
  *(float4*)(sst + (r * 2 + 1) * a.Cout + n) = make_float4(s2[0], s2[1], s2[2], s2[3]);
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * a.Cout; c += 256) {
    const int half = c / a.Cout, ch = c - half * a.Cout;
    float acc = 0.f;
    for (int qq = 0; qq < RPB; ++qq) acc += sst[(qq * 2 + half) * a.Cout + ch];
    rows_out[(long)blockIdx.x * 2 * a.Cout + c] = acc;
  }
}

// Split-K reduce fused with the decoder's bilinear x2 upsample (eval; serving at N = 1): a block owns
// UP_TY output rows of one image x UP_CG channels. Phase 1 reduces the slices of the (at most
// UP_TY / 2 + 2) source rows those output rows read -- same summation and epilogue as
// conv_splitk_reduce_kernel, so the low-resolution output y is written bitwise as there (rows shared by
// two bands are written twice with equal values) -- into LDS as bf16; phase 2 interpolates the output
// rows from LDS with the arithmetic of upsample2_fwd_kernel (csrc/pool_up.hip). The low-res tensor is
// never re-read from memory and the upsample launch disappears.
#define UP_TY RDP_UP_TY
#define UP_CG RDP_UP_CG
__global__ __launch_bounds__(256) void conv_splitk_reduce_up_kernel(const ConvArgs a) {
  extern __shared__ uint32_t srcs[];  // [source row][W][UP_CG / 2] packed bf16 pairs
  const int nb = (a.uH + UP_TY - 1) / UP_TY;
  const int img = blockIdx.x / nb, band = blockIdx.x - img * nb;
  const int c0 = blockIdx.y * UP_CG;
  const int Y0 = band * UP_TY, Y1 = min(a.uH, Y0 + UP_TY);
  int sy_lo = a.H, sy_hi = -1;
  for (int Y = Y0; Y < Y1; ++Y) {
    const int uy = Y - a.uoy;
    if (uy < 0 || uy >= 2 * a.H) continue;
    int y0, y1;
    float ly;
    up_src(uy, a.H, a.urh, y0, y1, ly);
    sy_lo = min(sy_lo, y0);
    sy_hi = max(sy_hi, y1);
  }
  const int nrows = sy_hi >= sy_lo ? sy_hi - sy_lo + 1 : 0;
  const auto rk = make_rsrc(a.kslab, (uint32_t)((long)a.ksplit * a.M * a.Cout * 4));
  const uint32_t sstride = (uint32_t)a.M * (uint32_t)a.Cout * 4u;
  constexpr int NQ = UP_CG / 4;  // 4-channel quads per block
  for (int it = threadIdx.x; it < nrows * a.W * NQ; it += 256) {
    const int q = it % NQ, px = it / NQ;
    const int r = px / a.W, x = px - r * a.W;
    const int m = (img * a.H + sy_lo + r) * a.W + x;
    const int n = c0 + 4 * q;
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t base = ((uint32_t)m * (uint32_t)a.Cout + (uint32_t)n) * 4u;
    for (int sp0 = 0; sp0 < a.ksplit; sp0 += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t off = sp0 + u < a.ksplit ? base + (uint32_t)(sp0 + u) * sstride : RDP_OOB;
        v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0));
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u & 3] += v[u];
    }
    f32x4 o = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    const float4 sc = *(const float4*)(a.escale + n), sh = *(const float4*)(a.eshift + n);
    o[0] = fmaf(o[0], sc.x, sh.x); o[1] = fmaf(o[1], sc.y, sh.y);
    o[2] = fmaf(o[2], sc.z, sh.z); o[3] = fmaf(o[3], sc.w, sh.w);
    if (a.erelu) {
      o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f); o[2] = fmaxf(o[2], 0.f); o[3] = fmaxf(o[3], 0.f);
    }
    const uint2 w = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
    *(uint2*)(a.y1 + (long)m * a.ypitch1 + n) = w;
    srcs[(px * NQ + q) * 2] = w.x;
    srcs[(px * NQ + q) * 2 + 1] = w.y;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < (Y1 - Y0) * a.uW * NQ; it += 256) {
    const int q = it % NQ, t = it / NQ;
    const int X = t % a.uW, Y = Y0 + t / a.uW;
    const int uy = Y - a.uoy, ux = X - a.uox;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (!(uy < 0 || ux < 0 || uy >= 2 * a.H || ux >= 2 * a.W)) {
      int y0, y1, x0, x1;
      float ly, lx;
      up_src(uy, a.H, a.urh, y0, y1, ly);
      up_src(ux, a.W, a.urw, x0, x1, lx);
      auto ld = [&](int yy, int xx, float* f) {
        const int i = (((yy - sy_lo) * a.W + xx) * NQ + q) * 2;
        unpack4(make_uint2(srcs[i], srcs[i + 1]), f);
      };
      float pa[4], pb[4], pc[4], pd[4];
      ld(y0, x0, pa); ld(y0, x1, pb); ld(y1, x0, pc); ld(y1, x1, pd);
      const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = hy * (hx * pa[k] + lx * pb[k]) + ly * (hx * pc[k] + lx * pd[k]);
    }
    *(uint2*)(a.up + ((long)(img * a.uH + Y) * a.uW + X) * a.upitch + c0 + 4 * q) =
        make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
  }
}

// The reduce + epilogue launch after a split-K conv (g: its geometry): returns the rows it reports; *pooled is set
// where it wrote the fused pool / upsample
static int launch_split_reduce(const ConvArgs& a, const RdpIgemmGeo& g, hipStream_t s, int* pooled) {
  if (g.up) {  // fused eval upsample: bands of UP_TY output rows x UP_CG channels
    const size_t lds = (size_t)(UP_TY / 2 + 2) * a.W * UP_CG * 2;
    hipLaunchKernelGGL(conv_splitk_reduce_up_kernel, dim3(g.rgrid, g.rgrid_y), dim3(256), lds, s, a);
    if (pooled) *pooled = 1;
    return g.rows;
  }
  if (g.pool && pooled) *pooled = 1;  // fused eval MaxPool2d(2): one work row per 2x2 window
  const int rpb = 256 / (a.Cout / 4);
  const size_t lds = (a.stats || g.bn) ? (size_t)rpb * 2 * a.Cout * sizeof(float) : 0;
  hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3(g.rgrid), dim3(256), lds, s, a, g.rgrid);
  if (g.bn && a.bnrows) *a.bnrows = g.rows;
  return g.rows;
}

template <int BM, int BN, int NWV = 4>
static int launch_cfg(ConvArgs a, long ws_limit, hipStream_t s, int* pooled = nullptr) {
  const RdpIgemmGeo g = rdp_igemm_geo(gemm_shape(a), BM, BN, a.kslab ? ws_limit : 0, 512, fuse_of(a));
  if (!g.fits) return -1;
  a.tilesN = g.tilesN; a.ntiles = g.ntiles; a.ksplit = g.ksplit; a.nks = g.nks;
  if (g.ksplit > 1) {
    hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, NWV>), dim3(g.grid), dim3(64 * NWV), 0, s, a);
    return launch_split_reduce(a, g, s, pooled);
  }
  a.pool = nullptr;  // the non-split epilogue does not pool / upsample (the caller launches them)
  a.up = nullptr;
  hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, NWV>), dim3(g.grid), dim3(64 * NWV), 0, s, a);
  return g.rows;
}

// The one RdpConv -> ConvArgs fill. ws: the split-K fp32 slab or nullptr; the fused pool / upsample / BN-backward
// operands are set where rdp_conv_fuse_ok allows them (they act only if the launch splits K).
static ConvArgs conv_args(const RdpConv& c, int taps, int packed, float* ws, const RdpConvFuse& fuse, int* pooled,
                          const RdpConvBnBwd& bn, int* bnrows) {
  const RdpConvFuseOk ok = rdp_conv_fuse_ok(c, fuse, pooled != nullptr, bn);
  ConvArgs a;
  a.x1 = (const u16*)c.x1; a.x2 = (const u16*)c.x2;
  a.xbytes1 = (uint32_t)c.xbytes1; a.xbytes2 = (uint32_t)c.xbytes2;
  a.C1 = c.C1; a.C2 = c.C2; a.pitch1 = c.pitch1; a.pitch2 = c.pitch2;
  a.w = (const u16*)c.w; a.wbytes = (uint32_t)c.wbytes; a.ldw = c.ldw;
  a.y1 = (u16*)c.y1; a.y2 = (u16*)c.y2; a.ybytes1 = (uint32_t)c.ybytes1; a.ybytes2 = (uint32_t)c.ybytes2;
  a.Cy1 = c.Cy1; a.ypitch1 = c.ypitch1; a.ypitch2 = c.ypitch2; a.stats = c.stats;
  a.escale = c.escale; a.eshift = c.eshift; a.erelu = c.erelu;
  a.N = c.N; a.H = c.H; a.W = c.W; a.Cout = c.Cout; a.M = c.N * c.H * c.W;
  a.taps = taps; a.packed = packed;
  a.cpt = packed ? 1 : (c.C1 + c.C2) / 64;
  a.nks = packed ? 2 : taps * a.cpt;
  a.ksplit = 1;
  a.kslab = ws;
  a.pool = ok.pool ? (u16*)fuse.pool : nullptr;
  a.ppitch = fuse.ppitch;
  a.up = ok.up ? (u16*)fuse.up : nullptr;
  a.upitch = fuse.upitch; a.uH = fuse.uH; a.uW = fuse.uW; a.uoy = fuse.uoy; a.uox = fuse.uox;
  a.urh = 2 * c.H > 1 ? (float)(c.H - 1) / (float)(2 * c.H - 1) : 0.f;  // = ac_scale (pool_up.hip)
  a.urw = 2 * c.W > 1 ? (float)(c.W - 1) / (float)(2 * c.W - 1) : 0.f;
  if (ok.bn) {
    a.bny = (const u16*)bn.bny; a.bnypitch = bn.bnypitch; a.bncoef = bn.bncoef; a.bnpart = bn.bnpart;
    a.bnrows = bnrows;
  }
  const FastDiv fhw = make_fastdiv((uint32_t)(c.H * c.W)), fw = make_fastdiv((uint32_t)c.W);
  a.fhw_m = fhw.m; a.fhw_s = fhw.s; a.fw_m = fw.m; a.fw_s = fw.s;
  return a;
}

extern "C" int rdp_conv_igemm(const RdpConv& c, int taps, int packed, int kernel, float* ws, long ws_elems,
                              const void* wfrag, long wfrag_bytes, const RdpConvFuse& fuse, int* pooled,
                              const RdpConvBnBwd& bn, int* bnrows, const RdpConvBnIn& in, hipStream_t s) {
  if (pooled) *pooled = 0;
  if (bnrows) *bnrows = 0;
  const bool has_ws = ws != nullptr && ws_elems > 0;
  const RdpConvPlan p = rdp_conv_plan(c, taps, packed, kernel, has_ws, ws_elems, fuse, pooled != nullptr, bn, in,
                                      wfrag ? wfrag_bytes : 0);
  switch (p.kernel) {
    case RDP_CONV_UNSUPPORTED: return -1;
    case RDP_CONV_FIRST: return rdp_conv_first(c, s);
    case RDP_CONV_ROWBAND: {
      RdpConv cw = c;
      if (p.rowband_mode) { cw.w = wfrag; cw.wbytes = wfrag_bytes; cw.ldw = 0; }
      void* const pool = p.pool_fused ? fuse.pool : nullptr;
      const int r = rdp_conv_rowband_ex(cw, pool, pool ? rdp_conv_pool_bytes(c, fuse) : 0, fuse.ppitch, p.rowband_mode, s);
      if (r == 1) *pooled = 1;
      return r < 0 ? -1 : 0;
    }
    case RDP_CONV_RING: {
      const int r = rdp_conv_ring(c, p.ring_form, fuse, bn, in, s);
      if (r >= 0 && p.pool_fused) *pooled = 1;
      if (r >= 0 && p.bn_rows && bnrows) *bnrows = r;
      return r;
    }
    case RDP_CONV_RING2:
    case RDP_CONV_RING2X2: {
      RdpConv h = rdp_ring2_sources(c);  // one launch per 64 output channels: the block with the slice offsets applied
      int r = -1;
      for (int co0 = 0; co0 < c.Cout; co0 += 64) {
        h.w = (const u16*)c.w + (long)co0 * c.ldw;
        h.wbytes = c.wbytes - (long)co0 * c.ldw * 2;
        h.y1 = (u16*)c.y1 + co0;
        h.ybytes1 = c.ybytes1 - (long)co0 * 2;
        h.escale = c.escale ? c.escale + co0 : nullptr;
        h.eshift = c.eshift ? c.eshift + co0 : nullptr;
        r = rdp_conv_ring2(h, 256, c.Cout, co0, s);
        if (r < 0) break;
      }
      return r;
    }
    case RDP_CONV_HALO: return rdp_conv_halo(c, s);
    default: break;
  }
  const ConvArgs a = conv_args(c, taps, packed, has_ws ? ws : nullptr, fuse, pooled, bn, bnrows);
  const long ws_limit = rdp_conv_ws_limit(has_ws, ws_elems);
  switch (p.kernel) {
    case RDP_CONV_PP256: return launch_pp<256>(a, s);
    case RDP_CONV_PP128: return launch_pp<128>(a, s);
    case RDP_CONV_PPSK128: return launch_pp<128>(a, s, p.ksplit, pooled);
    case RDP_CONV_PPSK256: return launch_pp<256>(a, s, p.ksplit, pooled);
    case RDP_CONV_IGEMM8_128: return launch_cfg<128, 128, 8>(a, ws_limit, s, pooled);
    case RDP_CONV_IGEMM8_256: return launch_cfg<256, 64, 8>(a, ws_limit, s, pooled);
    case RDP_CONV_IGEMM4_128: return launch_cfg<128, 128>(a, ws_limit, s, pooled);
    case RDP_CONV_IGEMM4_256: return launch_cfg<256, 64>(a, ws_limit, s, pooled);
    default: return -1;
  }
}
