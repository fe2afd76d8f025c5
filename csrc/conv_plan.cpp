// The conv plan: see conv_plan.h. Host integer arithmetic only; the A/B environment knobs are read once.
#include "conv_plan.h"

#include <stdlib.h>

#include <algorithm>

namespace {

constexpr long kMaxBytes = 1L << 31;  // every buffer descriptor's reach

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

int ilog2_exact(long v) {
  int s = 0;
  while ((1L << s) < v) ++s;
  return (1L << s) == v ? s : -1;
}

bool rowband_on() {
  static const int on = env_int("RDP_ROWBAND", 1);
  return on != 0;
}

bool pp_split_enabled() {  // RDP_PP_SPLIT=0: the 128 x 128 split-K kernel instead (A/B)
  static const int on = env_int("RDP_PP_SPLIT", 1);
  return on != 0;
}

bool splitk_bnred_on() {  // RDP_SPLITK_BNRED=0: the split-K reduce leaves the BN-backward rows to a separate pass
  static const int on = env_int("RDP_SPLITK_BNRED", 1);
  return on != 0;
}

// the row-ring grid: blocks of pairs_per_block row pairs
void ring_grid(RdpRingGeo& g, int N, int H, int W, int max_blocks) {
  g.WS = W / 64;
  g.nrows = N * g.WS * H;
  g.npairs = g.nrows / 2;
  const int blocks = std::max(1, std::min(max_blocks > 0 ? max_blocks : 256, g.npairs));
  g.pairs_per_block = (g.npairs + blocks - 1) / blocks;
  g.grid = (g.npairs + g.pairs_per_block - 1) / g.pairs_per_block;
}

// The reduce + epilogue launch after a split-K conv: one stats row per block (<= 512); the fused upsample runs
// bands of RDP_UP_TY output rows x RDP_UP_CG channels, the fused pool one work row per 2x2 window
void split_reduce(RdpIgemmGeo& r, const RdpGemmShape& g, RdpConvFuseOk ok) {
  const int rpb = 256 / (g.Cout / 4);
  int nblk = std::min((g.M + rpb - 1) / rpb, 512);
  r.pool = ok.pool;
  r.up = ok.up;
  if (ok.up) {
    r.rgrid = g.N * ((g.uH + RDP_UP_TY - 1) / RDP_UP_TY);
    r.rgrid_y = g.Cout / RDP_UP_CG;
    r.rows = 0;
    return;
  }
  if (ok.pool) nblk = std::min((g.M / 4 + rpb - 1) / rpb, 2048);
  r.bn = !g.stats && ok.bn && !ok.pool;
  r.rgrid = nblk;
  r.rows = ok.pool ? 0 : nblk;  // (the pooling reduce is eval only: it writes no partial rows)
}

}  // namespace

const RdpConvKernelName rdp_conv_kernel_names[] = {
    {RDP_CONV_AUTO, "AUTO"},           {RDP_CONV_HALO, "HALO"},
    {RDP_CONV_IGEMM8_128, "IGEMM8_128"}, {RDP_CONV_IGEMM8_256, "IGEMM8_256"},
    {RDP_CONV_PP256, "PP256"},         {RDP_CONV_PP128, "PP128"},
    {RDP_CONV_RING, "RING"},           {RDP_CONV_PPSK128, "PPSK128"},
    {RDP_CONV_PPSK256, "PPSK256"},     {RDP_CONV_FIRST, "FIRST"},
    {RDP_CONV_RING2, "RING2"},         {RDP_CONV_RING2X2, "RING2X2"},
    {RDP_CONV_ROWBAND, "ROWBAND"},     {RDP_CONV_IGEMM4_128, "IGEMM4_128"},
    {RDP_CONV_IGEMM4_256, "IGEMM4_256"},
};
const int rdp_conv_kernel_count = sizeof(rdp_conv_kernel_names) / sizeof(rdp_conv_kernel_names[0]);

const char* rdp_conv_kernel_name(int kernel) {
  for (int i = 0; i < rdp_conv_kernel_count; ++i)
    if (rdp_conv_kernel_names[i].kernel == kernel) return rdp_conv_kernel_names[i].name;
  return "UNSUPPORTED";
}

// ---- first layer -----------------------------------------------------------------------------------------------
RdpFirstGeo rdp_first_geo(const RdpConv& c, int taps, int packed) {
  RdpFirstGeo g;
  if (!packed || c.C1 != 8 || c.C2 != 0 || c.x2 != nullptr || taps != 9 || c.Cout != 64 || c.y2 != nullptr) return g;
  if (c.pitch1 < 4 || c.wbytes < 64l * 128 * 2 || c.ypitch1 < 64 || c.ypitch1 % 8) return g;
  if (c.xbytes1 >= kMaxBytes || c.ybytes1 >= kMaxBytes) return g;
  const int M = c.N * c.H * c.W;
  g.nseg = (M + 63) / 64;
  g.grid = std::max(1, std::min((g.nseg + 3) / 4, 512));  // one stats row per block
  g.rows = c.stats ? g.grid : 0;
  g.fits = true;
  return g;
}

// ---- row band --------------------------------------------------------------------------------------------------
long rdp_rowband_bytes(int N, int H, int W, int Cin, int Cout, int pool) {
  const int R = pool && H % 2 == 0 && 2 * W <= 64 ? 2 : 1;
  const long wb = (long)Cout * 9 * Cin * 2, xb = (long)N * H * W * Cin * 2;
  return wb * ((long)N * H / R) + xb * 9 * (Cout / 32);
}

bool rdp_rowband_auto(int N, int H, int W, int Cin, int Cout, bool pool) {
  if (!rowband_on() || (long)N * H * W > 4096 || W > 64 || Cin < 128 || Cout < 64) return false;
  if (pool && !(H % 2 == 0 && 2 * W <= 64)) return false;
  // (the estimate without the pool's two-row blocks: with or without a pool the same kernel runs, so the
  // two calls give bitwise the same activations)
  return rdp_rowband_bytes(N, H, W, Cin, Cout, 0) <= 160000000L;
}

// With the fragment-major weight copy (1 KiB contiguous per MFMA fragment: 8 full lines per load instead of
// 16 half lines) a weight byte costs about half an activation byte (scripts/rowband_bench.py variant 17:
// 16^2 512 -> 512 8.8 vs 14.6 us on OHWI weights, 32^2 256 -> 512 13.2 vs 18.9): the row-band kernel up to
// 250 MB of weighted operand bytes, every <= 64^2 layer of the U-Net but the two long-K decoder convs
// (32^2 1024 -> 512, 64^2 512 -> 256).
int rdp_rowband_frag_mode(int N, int H, int W, int C1, int C2, int Cout) {
  const int Cin = C1 + C2;
  if (!rowband_on() || W < 16 || Cin < 64 || Cout < 64 || Cout % 32 || C1 % 32 || C2 % 32) return 0;
  if (ilog2_exact(W) < 0 || ilog2_exact(Cin / 32) < 0) return 0;
  const long M = (long)N * H * W;
  const long wb = (long)Cout * 9 * Cin * 2, xb = M * Cin * 2;
  static const long xmax = [] {
    const char* e = getenv("RDP_ROWBAND_X_MAXPIX");  // 0 turns the activation-staged kernel off
    return e ? atol(e) : 65536L;  // (the work bound below decides; up3.conv2 at N = 2: 20.0 vs 32.5 us)
  }();
  // (64 input channels stay on the split-K GEMM: 128^2 64 -> 128 18.0 vs 11.5 us, four waves staging one chunk)
  const bool xch = (Cin / 32) % 8 == 0 || Cin == 128;
  if (xch && M <= xmax && W <= 256) {  // activation-staged (x read ~3x instead of 9x)
    // ... while its work (blocks x K, the launch's own tiling) stays within about two waves of 512
    // blocks: past that the GEMM wins (scripts/rowband_bench.py --batch 1 / 2 / 4, every <= 128^2 layer of
    // the U-Net: e.g. up1.conv1 17.9 vs 26.9 us at N = 1 but 44.9 vs 38.8 at N = 2, down2.conv1 20.9 vs
    // 25.3 at N = 2 but 38.9 vs 20.2 at N = 4; 128-channel inputs, staged in 4 chunks, cross over earlier)
    const int WB = W < 32 ? W : 32, segs = W / WB;
    const bool r2 = H % 2 == 0 && (long)N * (H / 2) * segs * (Cout / 32) >= 256;
    const long blocks = (long)N * (H / (r2 ? 2 : 1)) * segs * (Cout / 32);
    const long work = blocks * 9 * Cin;
    if (work <= ((Cin / 32) % 8 == 0 ? 2500000L : 1300000L)) return 2;
    return 0;
  }
  if (M > 4096 || W > 64) return 0;
  return wb * ((long)N * H) / 2 + xb * 9 * (Cout / 32) <= 250000000L ? 1 : 0;
}

RdpRowbandGeo rdp_rowband_geo(const RdpConv& c, bool pool, long pbytes, int ppitch, int wfrag) {
  RdpRowbandGeo g;
  const int Cin = c.C1 + c.C2;
  g.cshift = ilog2_exact(Cin / 32);
  g.wshift = ilog2_exact(c.W);
  if (c.C1 % 32 || c.C2 % 32 || Cin < 64 || Cin % 32 || g.cshift < 0 || g.wshift < 4 ||
      c.W > (wfrag == 2 ? 256 : 64) || c.Cout % 32)
    return g;
  if (!c.escale || !c.eshift || (!wfrag && c.ldw < 9 * Cin) || (wfrag && c.wbytes < (long)c.Cout * 9 * Cin * 2) ||
      (c.C2 && !c.x2))
    return g;
  if (c.pitch1 % 8 || (c.C2 && c.pitch2 % 8) || c.ypitch1 % 4) return g;
  if (c.xbytes1 >= kMaxBytes || c.xbytes2 >= kMaxBytes || c.wbytes >= kMaxBytes || c.ybytes1 >= kMaxBytes ||
      pbytes >= kMaxBytes)
    return g;
  g.T = 9 * Cin / 32;
  if (wfrag == 2) {  // the activation-staged kernel: 32-channel chunks (a multiple of 8, or 2 / 4)
    if ((Cin / 32) % 8 && Cin != 64 && Cin != 128) return g;
    const int WB = c.W < 32 ? c.W : 32;
    g.pools = pool && c.H % 2 == 0 && ppitch % 4 == 0;
    // two-row tiles (each block's weight slice serves twice the pixels) wherever that grid still has >= 256
    // blocks: up1.conv1 22.4 -> 18.2 us, up2.conv1 24.5 -> 21.9, down3.conv1 7.8 -> 6.9 (at 128 blocks, the
    // 16^2 and 32^2 -> 256 convs, one-row tiles stay faster)
    static const int r2_on = env_int("RDP_ROWBAND_R2", 1);
    const bool r2 = r2_on && c.H % 2 == 0 && (long)c.N * (c.H / 2) * (c.W / WB) * (c.Cout / 32) >= 256;
    g.R = g.pools || r2 ? 2 : 1;
    g.segs = c.W / WB;
    g.PB = g.R * WB;
    g.bands = c.H / g.R;
    g.grid = c.N * g.bands * g.segs * (c.Cout / 32);
    g.fits = g.PB == 16 || g.PB == 32 || g.PB == 64;
    return g;
  }
  // the pool needs two rows per block: only where that block is <= 64 pixels (else the caller pools)
  g.pools = pool && c.H % 2 == 0 && ppitch % 4 == 0 && 2 * c.W <= 64;
  g.R = g.pools ? 2 : 1;
  g.PB = g.R * c.W;
  g.bands = c.H / g.R;
  g.grid = c.N * g.bands * (c.Cout / 32);
  g.fits = g.PB == 16 || g.PB == 32 || g.PB == 64;
  return g;
}

// ---- row ring --------------------------------------------------------------------------------------------------
RdpRingGeo rdp_ring_geo(const RdpConv& c, RdpRingForm form, int ppitch, int max_blocks, const RdpConvBnBwd& bn,
                        const RdpConvBnIn& in) {
  RdpRingGeo g;
  if (c.C1 != 64 || c.W % 64 || c.H % 2 || c.ldw < 576) return g;
  if (c.xbytes1 >= kMaxBytes || c.wbytes >= kMaxBytes) return g;
  if (form == RDP_RING_HEAD || form == RDP_RING_POOL) {  // eval, 64 -> 64
    if (c.Cout != 64 || !c.escale || !c.eshift) return g;
    if (form == RDP_RING_POOL && (ppitch % 4 || c.ybytes1 >= kMaxBytes || c.y2 || c.Cy1 != 64)) return g;
  } else {
    const bool unfusable = c.escale || c.y2 || c.Cout != 64;  // what neither fused training form takes
    const bool bn_ok = bn.bny && bn.bncoef && bn.bnpart && bn.bnypitch % 4 == 0 && !c.stats;
    if (form == RDP_RING_BNRED && (!bn_ok || unfusable)) return g;
    if (form == RDP_RING_BNIN && (!in.iscale || !in.ishift || unfusable)) return g;
    if (form == RDP_RING_BNIN && in.aout && (in.abytes >= kMaxBytes || in.apitch % 8)) return g;
    if ((c.Cout != 64 && c.Cout != 128) || c.Cy1 % 32) return g;
    if (c.y2 == nullptr && c.Cy1 != c.Cout) return g;
    if (c.ybytes1 >= kMaxBytes || c.ybytes2 >= kMaxBytes) return g;
  }
  ring_grid(g, c.N, c.H, c.W, max_blocks);
  // one partial row per (block, pixel group): 4 groups of 32 pixels at 64 couts, 2 of 64 at 128
  g.rows = form == RDP_RING_HEAD || form == RDP_RING_POOL ? 0 : c.Cout == 128 ? g.grid * 2 : g.grid * 4;
  g.fits = true;
  return g;
}

RdpRingGeo rdp_ring2_geo(const RdpConv& c, int max_blocks, int cout_total, int co0) {
  RdpRingGeo g;
  if (c.W % 64 || c.H % 2 || c.ldw < 1152 || c.ypitch1 % 8 || c.pitch1 % 8 || c.pitch2 % 8) return g;
  if (c.xbytes1 >= kMaxBytes || c.xbytes2 >= kMaxBytes || c.ybytes1 >= kMaxBytes || c.wbytes >= kMaxBytes) return g;
  if ((c.escale == nullptr) != (c.eshift == nullptr)) return g;
  if (cout_total < 64 || co0 < 0 || co0 + 64 > cout_total) return g;
  ring_grid(g, c.N, c.H, c.W, max_blocks);
  g.rows = g.grid * 4;
  g.fits = true;
  return g;
}

RdpConv rdp_ring2_sources(const RdpConv& c) {
  RdpConv h = c;
  if (c.C1 == 128 && c.C2 == 0 && c.x2 == nullptr) {  // the second source = the upper half of the one tensor
    h.x2 = (const char*)c.x1 + 128;
    h.xbytes2 = c.xbytes1 - 128;
    h.pitch2 = c.pitch1;
  }
  return h;
}

// ---- halo tiles ------------------------------------------------------------------------------------------------
RdpHaloGeo rdp_halo_geo(const RdpConv& c, int taps, int packed) {
  RdpHaloGeo g;
  if (taps != 9 || packed || c.C1 % 64 || c.C2 % 64 || c.C1 == 0 || c.Cout % 64) return g;
  if (c.W % 64 == 0 && c.H % 4 == 0) { g.TC = 64; g.TR = 4; }
  else if (c.W % 32 == 0 && c.H % 8 == 0) { g.TC = 32; g.TR = 8; }
  else if (c.W % 16 == 0 && c.H % 16 == 0) { g.TC = 16; g.TR = 16; }
  else return g;
  // 8 waves per block either way (2 per SIMD): BN = 128 -> 4 (pixels) x 2 (couts), BN = 64 -> 8 x 1
  const bool wide = c.Cout % 128 == 0;
  g.WM = wide ? 4 : 8;
  g.WN = wide ? 2 : 1;
  g.tilesH = c.H / g.TR;
  g.tilesW = c.W / g.TC;
  g.tilesN = c.Cout / (64 * g.WN);
  const int tilesM = c.N * g.tilesH * g.tilesW;
  g.ntiles = tilesM * g.tilesN;
  g.grid = std::min(g.ntiles, 256);
  g.rows = tilesM * g.WM;  // one per (256-pixel tile, wave row)
  g.shape = g.ntiles > 0;
  if (c.ldw < 9 * (c.C1 + c.C2) || c.Cy1 % 4) return g;
  if (c.xbytes1 >= kMaxBytes || c.xbytes2 >= kMaxBytes || c.ybytes1 >= kMaxBytes || c.ybytes2 >= kMaxBytes ||
      c.wbytes >= kMaxBytes)
    return g;
  g.fits = g.shape;
  return g;
}

// ---- implicit GEMM / ping-pong ---------------------------------------------------------------------------------
RdpConvFuseOk rdp_conv_fuse_ok(const RdpConv& c, const RdpConvFuse& fuse, bool want_fused, const RdpConvBnBwd& bn) {
  RdpConvFuseOk ok;
  ok.pool = fuse.pool != nullptr && want_fused && c.stats == nullptr && c.y2 == nullptr && c.H % 2 == 0 && c.W % 2 == 0;
  // fused upsample needs the eval epilogue, 16-channel groups and the LDS band (<= 64 KB). Measured
  // (serving frame, N = 1): it wins only at the 16^2 bottleneck (6.9 us vs 4.8 + 4.8 us); at 32^2 /
  // 64^2 / 128^2 the banded two-phase kernel is slower than reduce + upsample (10.9 / 13.2 / 15.4 vs
  // 9.8 / 10.3 / 10.6 us; 2-row bands x 8 channels were slower still), so larger maps take the
  // separate upsample launch.
  ok.up = fuse.up != nullptr && want_fused && fuse.pool == nullptr && c.stats == nullptr && c.y2 == nullptr &&
          c.escale != nullptr && c.eshift != nullptr && c.Cout % RDP_UP_CG == 0 && fuse.upitch % 4 == 0 &&
          (long)(RDP_UP_TY / 2 + 2) * c.W * RDP_UP_CG * 2 <= 65536 && fuse.uH >= 2 * c.H && fuse.uW >= 2 * c.W &&
          (long)c.H * c.W <= 256;
  ok.bn = splitk_bnred_on() && bn.bnpart && bn.bny && bn.bncoef && !c.stats && !c.escale && c.y2 == nullptr &&
          c.Cy1 == c.Cout && bn.bnypitch % 4 == 0 && fuse.pool == nullptr && fuse.up == nullptr;
  return ok;
}

int rdp_choose_ksplit(int ntiles, int nks, int M, int Cout, int packed, long ws_elems) {
  const bool pow2 = Cout >= 64 && Cout <= 1024 && (Cout & (Cout - 1)) == 0;  // reduce kernel's groups
  int ks = 1;
  if (!pow2 || packed || ntiles >= 192) return 1;
  for (int d = 2; d <= nks / 4; ++d) {
    if (nks % d) continue;
    if ((long)d * M * Cout > ws_elems) break;
    ks = d;
    if (ntiles * d >= 256) break;
  }
  return ks;
}

int rdp_pp_split(int M, int Cout, int BN, int nks, long ws_elems) {
  constexpr int kMinKs = 8;
  // (the split-K reduce kernel maps a power-of-two channel count, 64..1024, onto its threads)
  if (Cout % BN || Cout > 1024 || (Cout & (Cout - 1))) return 0;
  const long tiles = (long)(M + 255) / 256 * (Cout / BN);
  if (tiles >= 256) return 0;
  for (int d = 2; d <= nks / kMinKs; ++d) {
    if (nks % d) continue;
    if ((long)d * M * Cout > ws_elems) return 0;
    if (tiles * d >= 256) return d;
  }
  return 0;
}

RdpIgemmGeo rdp_igemm_geo(const RdpGemmShape& g, int BM, int BN, long ws_elems, int max_blocks, RdpConvFuseOk ok) {
  RdpIgemmGeo r;
  if (g.Cout % BN) return r;
  r.tilesN = g.Cout / BN;
  r.ntiles = (g.M + BM - 1) / BM * r.tilesN;
  r.nks = g.nks;
  r.ksplit = ws_elems > 0 ? rdp_choose_ksplit(r.ntiles, g.nks, g.M, g.Cout, g.packed, ws_elems) : 1;
  if (r.ksplit > 1) {
    r.nks /= r.ksplit;
    r.ntiles *= r.ksplit;
    r.grid = std::min(r.ntiles, max_blocks);
    split_reduce(r, g, ok);
    r.fits = true;
    return r;
  }
  // (the non-split epilogue does not pool / upsample: the caller launches them)
  r.grid = std::min(r.ntiles, max_blocks);
  // the per-block stats rows need every block to keep one channel tile (see the kernel)
  if (g.stats && r.grid % r.tilesN) return r;
  r.rows = r.grid / r.tilesN * (BM / 64);  // one per (block group, wave row)
  r.fits = true;
  return r;
}

RdpIgemmGeo rdp_pp_geo(const RdpGemmShape& g, int BN, int ksplit, bool has_ws, RdpConvFuseOk ok) {
  RdpIgemmGeo r;
  if (g.packed || g.Cout % BN || g.Cy1 % 32) return r;
  r.tilesN = g.Cout / BN;
  r.ntiles = (g.M + 255) / 256 * r.tilesN;
  r.nks = g.nks;
  if (ksplit > 1) {
    if (!has_ws || g.nks % ksplit) return r;
    r.ksplit = ksplit;
    r.nks /= ksplit;
    r.ntiles *= ksplit;
    r.grid = std::min(r.ntiles, 256);
    split_reduce(r, g, ok);
    r.fits = true;
    return r;
  }
  // one persistent block per CU (512 blocks or one block per tile, which let the dispatcher balance
  // the tiles around the concurrent wgrads, measured 0.8 % / 1.7 % slower: profiles/dead_ends.md)
  r.grid = std::min(r.ntiles, 256);
  if (g.stats && r.grid % r.tilesN) return r;
  r.rows = r.grid / r.tilesN * 2;
  r.fits = true;
  return r;
}

// ---- ConvTranspose2d on the ping-pong kernel -------------------------------------------------------------------
namespace {

// 256-pixel tiles x BN channels on one persistent block per CU, taken only where they fill the chip
RdpUpTGeo upT_tile(const RdpConv& c, int taps, int Cin, bool wide_only_long_k) {
  RdpUpTGeo u;
  RdpGemmShape g;
  g.M = c.N * c.H * c.W; g.Cout = c.Cout; g.Cy1 = c.Cout; g.nks = taps * (Cin / 64); g.N = c.N;
  const long mt = (long)(g.M + 255) / 256;
  if (c.Cout % 256 == 0 && mt * (c.Cout / 256) >= 256) u.BN = 256;
  else if ((!wide_only_long_k || Cin >= 128) && mt * (c.Cout / 128) >= 256) u.BN = 128;
  else return u;
  const RdpIgemmGeo r = rdp_pp_geo(g, u.BN, 1, false, RdpConvFuseOk{});
  u.fits = r.fits;
  u.grid = r.grid;
  return u;
}

bool upT_placed(const RdpConv& c, const RdpUpT& t) {
  return t.oy >= 0 && t.ox >= 0 && 2 * c.H + t.oy <= t.H2 && 2 * c.W + t.ox <= t.W2;
}

}  // namespace

RdpUpTGeo rdp_upT_fwd_geo(const RdpConv& c, const RdpUpT& t) {
  const int C = c.Cout / 4, Cin = c.C1;
  if (c.Cout % 4 || C < 64 || C > 512 || (C & (C - 1)) || Cin % 64 || c.ldw < Cin || c.ypitch1 % 8 || !upT_placed(c, t))
    return RdpUpTGeo{};
  if (c.xbytes1 >= kMaxBytes || c.ybytes1 >= kMaxBytes || c.wbytes >= kMaxBytes) return RdpUpTGeo{};
  RdpUpTGeo u = upT_tile(c, 1, Cin, true);
  u.tlc = ilog2_exact(C);
  return u;
}

RdpUpTGeo rdp_upT_dgrad_geo(const RdpConv& c, const RdpUpT& t) {
  const int C = c.C1, Cin = c.Cout;
  if (C % 64 || Cin % 128 || c.ldw < 4 * C || !upT_placed(c, t)) return RdpUpTGeo{};
  if (c.xbytes1 >= kMaxBytes || c.ybytes1 >= kMaxBytes || c.wbytes >= kMaxBytes) return RdpUpTGeo{};
  return upT_tile(c, 4, C, false);
}

RdpUpTGeo rdp_upT_geo_dense(bool fwd, int N, int h, int w, int Cin, int C, const RdpUpT& t) {
  static char mark;
  const long lo = (long)N * h * w * Cin * 2, hi = (long)N * t.H2 * t.W2 * C * 2;
  RdpConv c;
  c.N = N; c.H = h; c.W = w;
  c.x1 = &mark; c.w = &mark; c.y1 = &mark;
  c.wbytes = 4L * C * Cin * 2;
  if (fwd) {  // x [N][h][w][Cin] -> u [N][H2][W2][C]
    c.C1 = c.pitch1 = c.ldw = Cin; c.xbytes1 = lo;
    c.Cout = 4 * C; c.Cy1 = c.ypitch1 = C; c.ybytes1 = hi;
    return rdp_upT_fwd_geo(c, t);
  }
  c.C1 = c.pitch1 = C; c.ldw = 4 * C; c.xbytes1 = hi;  // du [N][H2][W2][C] -> dx [N][h][w][Cin]
  c.Cout = c.Cy1 = c.ypitch1 = Cin; c.ybytes1 = lo;
  return rdp_upT_dgrad_geo(c, t);
}

// ---- the weight gradients --------------------------------------------------------------------------------------
const RdpConvKernelName rdp_wgrad_kernel_names[] = {
    {RDP_WGRAD_AUTO, "AUTO"},       {RDP_WGRAD_RING, "RING"}, {RDP_WGRAD_PACKED, "PACKED"},     {RDP_WGRAD_UPT, "UPT"},
    {RDP_WGRAD_GENERIC, "GENERIC"}, {RDP_WGRAD_HALO, "HALO"}, {RDP_WGRAD_FIRST_BN, "FIRST_BN"},
};
const int rdp_wgrad_kernel_count = sizeof(rdp_wgrad_kernel_names) / sizeof(rdp_wgrad_kernel_names[0]);

const char* rdp_wgrad_kernel_name(int kernel) {
  for (int i = 0; i < rdp_wgrad_kernel_count; ++i)
    if (rdp_wgrad_kernel_names[i].kernel == kernel) return rdp_wgrad_kernel_names[i].name;
  return "UNSUPPORTED";
}

bool rdp_wgrad_halo_shape(int H, int W, bool forced) {
  return W % 64 == 0 || (W >= (forced ? 8 : 32) && 64 % W == 0 && (H * W) % 64 == 0);
}

RdpWgradSplit rdp_wgrad_pixel_split(long M, int splits) {
  RdpWgradSplit s;
  s.want = std::max(1, splits);
  const long pps = ((M + s.want - 1) / s.want + 63) / 64 * 64;
  s.per_split = (int)pps;
  s.splits = pps > 0 ? (int)((M + pps - 1) / pps) : 0;
  return s;
}

RdpWgradSplit rdp_wgrad_halo_split(int nseg, int tiles, int BN, long max_splits) {
  RdpWgradSplit s;
  const int target = BN == 64 ? 512 : 256;
  s.want = std::max(1, (target + tiles - 1) / tiles);
  s.want = std::min<long>(s.want, std::max(1, nseg));
  s.want = std::min(s.want, max_splits);
  if (s.want < 1) return s;
  s.per_split = (int)((nseg + s.want - 1) / s.want);
  s.splits = s.per_split > 0 ? (nseg + s.per_split - 1) / s.per_split : 0;
  return s;
}

RdpWgradReduce rdp_wgrad_reduce_geo(int splits, int Cout, int ncols_pad, int taps, int cin_pad, int cin_real) {
  RdpWgradReduce r;
  const long E = (long)Cout * ncols_pad;  // multiple of 4 (Cout % 64 == 0)
  const long chunks = (E / 4 + 255) / 256;
  r.G = (int)std::min<long>(std::min<long>(splits, 32), std::max<long>(1, (1024 + chunks - 1) / std::max(1L, chunks)));
  if (splits <= 8) r.G = splits;
  r.grid1 = r.G < splits ? (int)chunks : 0;
  const long total = (long)Cout * taps * cin_real;
  r.vec = cin_real % 4 == 0 && cin_pad % 4 == 0 ? 4 : 1;
  r.grid2 = (int)std::min<long>((total / r.vec + 255) / 256, 4096);
  return r;
}

namespace {

// the shared tail of every plan: the slab the splits use against the slab offered, the grid, the reduce
RdpWgradPlan wgrad_finish(RdpWgradPlan p, const RdpWgradSplit& s, long offered) {
  p.splits = s.splits;
  p.per_split = s.per_split;
  p.slab_elems = (long)s.splits * p.Cout * p.ncols_pad;
  p.grid = p.tiles * s.splits;
  p.status = p.slab_elems > offered             ? RDP_WGRAD_SLAB_SMALL
             : p.slab_elems * 4 >= kMaxBytes ? RDP_WGRAD_SLAB_2GIB
                                              : RDP_WGRAD_OK;
  p.reduce = rdp_wgrad_reduce_geo(s.splits, p.Cout, p.ncols_pad, p.taps, p.cin_pad, p.cin_out);
  return p;
}

}  // namespace

RdpWgradPlan rdp_wgrad_plan(const RdpWgrad& g, int kernel, int splits, const RdpUpT& upT, const RdpWgradBn& bn) {
  RdpWgradPlan p;
  const long M = (long)g.N * g.H * g.W;
  if (M < 1 || M >= kMaxBytes) return p;
  if (bn.da) {  // the first layer with its BN backward: one block per split, 64 couts x 80 columns
    if (kernel != RDP_WGRAD_AUTO || M % 64 || g.cin_real > 8 || g.cin_real < 1) return p;
    if (g.xbytes1 >= kMaxBytes || bn.dabytes >= kMaxBytes || bn.ybytes >= kMaxBytes) return p;
    if (g.pitch1 % 8 || bn.dapitch % 8 || bn.ypitch % 8) return p;
    p.kernel = RDP_WGRAD_FIRST_BN;
    p.BN = p.Cout = 64; p.taps = 9; p.tiles = 1; p.block = 256;
    p.ncols = 72; p.ncols_pad = RDP_WGRAD_FIRST_NCOLS; p.cin_pad = 8; p.cin_out = g.cin_real;
    return wgrad_finish(p, rdp_wgrad_pixel_split(M, splits), g.slab_elems);
  }
  int Cin = g.C1 + g.C2;
  p.Cout = g.Cout; p.taps = g.taps;
  if (upT.H2 > 0) {
    if (kernel != RDP_WGRAD_AUTO || g.taps != 4 || g.packed || g.C2 || g.C1 % 64 || g.Cout % 64 || g.C1 == 0) return p;
    if (upT.oy < 0 || upT.ox < 0 || 2 * g.H + upT.oy > upT.H2 || 2 * g.W + upT.ox > upT.W2) return p;
    if (g.xbytes1 >= kMaxBytes || g.dybytes >= kMaxBytes) return p;
    p.kernel = RDP_WGRAD_UPT;
  } else {
    if (kernel != RDP_WGRAD_AUTO && kernel != RDP_WGRAD_GENERIC && kernel != RDP_WGRAD_HALO) return p;
    if (g.packed) {
      if (g.C1 != 8 || g.C2 != 0 || g.taps != 9) return p;
      Cin = 8;
    } else if (g.C1 % 64 || g.C2 % 64 || Cin == 0) {
      return p;
    }
    if (g.Cout % 64 || g.Cout == 0 || g.taps < 1) return p;
    if (g.xbytes1 >= kMaxBytes || g.xbytes2 >= kMaxBytes || g.dybytes >= kMaxBytes) return p;
    // halo reuse: 3x3, whole 64-pixel row segments
    const bool forced = kernel == RDP_WGRAD_HALO;
    const bool halo = !g.packed && g.taps == 9 && kernel != RDP_WGRAD_GENERIC && rdp_wgrad_halo_shape(g.H, g.W, forced);
    if (forced && !halo) return p;
    if (halo) {
      p.BN = g.Cout % 128 == 0 ? 128 : 64;
      // the row ring: same split of the positions; only where the dispatcher chooses (a forced HALO is the halo kernel)
      const bool ring = kernel == RDP_WGRAD_AUTO && g.W % 64 == 0 && p.BN == 64;
      p.kernel = ring ? RDP_WGRAD_RING : RDP_WGRAD_HALO;
      p.multirow = !ring && g.W < 64;
      p.block = p.BN * 4;
      p.tiles = (Cin / 64) * (g.Cout / p.BN);
      p.ncols = p.ncols_pad = 9 * Cin;
      p.cin_pad = p.cin_out = Cin;
      const long row = (long)g.Cout * p.ncols;
      const RdpWgradSplit s = rdp_wgrad_halo_split((int)(M / 64), p.tiles, p.BN, g.slab_elems / row);
      if (s.want < 1) {
        p.status = RDP_WGRAD_SLAB_SMALL;
        return p;
      }
      return wgrad_finish(p, s, g.slab_elems);
    }
    p.kernel = g.packed ? RDP_WGRAD_PACKED : RDP_WGRAD_GENERIC;
  }
  // the generic kernel: 256 (tap, cin) columns x 64 couts per block, 8 waves
  p.BN = 64; p.block = 512;
  p.ncols = g.packed ? 72 : g.taps * Cin;
  p.ncols_pad = (p.ncols + 255) / 256 * 256;
  p.tiles = p.ncols_pad / 256 * (g.Cout / 64);
  p.cin_pad = Cin;
  p.cin_out = g.packed ? g.cin_real : Cin;
  return wgrad_finish(p, rdp_wgrad_pixel_split(M, splits), g.slab_elems);
}

RdpWgradPlan rdp_wgrad_plan_dense(const RdpWgradQuery& q) {
  static char mark;
  static float fmark;
  auto bytes = [&](int C) { return (long)q.N * q.H * q.W * C * 2; };
  RdpWgrad g;
  g.x1 = &mark; g.C1 = q.C1; g.pitch1 = q.C1; g.xbytes1 = bytes(q.C1);
  if (q.C2) { g.x2 = &mark; g.C2 = q.C2; g.pitch2 = q.C2; g.xbytes2 = bytes(q.C2); }
  g.dy = &mark; g.dypitch = q.Cout; g.dybytes = bytes(q.Cout);
  g.slab = &fmark; g.slab_elems = q.slab_elems; g.out = &fmark;
  g.N = q.N; g.H = q.H; g.W = q.W; g.Cout = q.Cout; g.taps = q.taps; g.packed = q.packed; g.cin_real = q.cin_real;
  RdpUpT t;
  if (q.upT) {  // du = the dense [N][2H][2W][C1] map
    t.H2 = 2 * q.H; t.W2 = 2 * q.W;
    g.xbytes1 = 4 * bytes(q.C1);
  }
  RdpWgradBn bn;
  if (q.first_bn) {
    bn.da = &mark; bn.y = &mark; bn.dapitch = bn.ypitch = 64; bn.dabytes = bn.ybytes = bytes(64);
    bn.coef = bn.coef2 = &fmark;
  }
  return rdp_wgrad_plan(g, q.kernel, q.splits, t, bn);
}

int rdp_wgrad_auto_splits(int N, int H, int W, int Cin, int Cout, int taps, int packed, int target_blocks) {
  const long M = (long)N * H * W;
  const long tiles = std::max(1L, (long)((packed ? 72 : taps * Cin) + 255) / 256 * (Cout / 64));
  return (int)std::max(1L, std::min((target_blocks + tiles - 1) / tiles, M / 2048));
}

extern "C" long rdp_conv_wgrad_slab_elems(int N, int H, int W, int Cin, int Cout, int taps, int packed, int splits) {
  const int ncols_pad = ((packed ? 72 : taps * Cin) + 255) / 256 * 256;
  return (long)rdp_wgrad_pixel_split((long)N * H * W, splits).splits * Cout * ncols_pad;
}

extern "C" long rdp_conv_wgrad_halo_slab_elems(int N, int H, int W, int Cin, int Cout) {
  if (Cin % 64 || Cout % 64 || Cin == 0 || Cout == 0 || !rdp_wgrad_halo_shape(H, W, false)) return 0;
  const int BN = Cout % 128 == 0 ? 128 : 64;
  const long nseg = (long)N * H * W / 64;
  return rdp_wgrad_halo_split((int)nseg, (Cin / 64) * (Cout / BN), BN, 1L << 40).want * Cout * 9L * Cin;
}

// ---- the plan --------------------------------------------------------------------------------------------------
RdpConvPlan rdp_conv_plan(const RdpConv& c, int taps, int packed, int kernel, bool has_ws, long ws_elems,
                          const RdpConvFuse& fuse, bool want_fused, const RdpConvBnBwd& bn, const RdpConvBnIn& in,
                          long wfrag_bytes) {
  RdpConvPlan p;
  const RdpConvPlan none;
  bool known = false;
  for (int i = 0; i < rdp_conv_kernel_count; ++i) known = known || rdp_conv_kernel_names[i].kernel == kernel;
  if (!known) return none;
  const bool autok = kernel == RDP_CONV_AUTO;
  const int Cin = c.C1 + c.C2;
  const bool wpool = fuse.pool != nullptr && want_fused, wup = fuse.up != nullptr && want_fused;

  // The row ring's fused training forms, before everything else. Neither has a grid threshold: the plain ring is
  // auto only from 256 row pairs (below), but a fused form also saves its layer a whole pass over the tensor, so
  // it runs at any size the kernel takes.
  const bool ring_ok = (autok || kernel == RDP_CONV_RING) && taps == 9 && !packed && c.C2 == 0 && c.x2 == nullptr;
  auto ring_fused = [&](RdpRingForm form) {
    const RdpRingGeo g = ring_ok ? rdp_ring_geo(c, form, 0, 256, bn, in) : RdpRingGeo{};
    if (g.fits) {
      p.kernel = RDP_CONV_RING;
      p.ring_form = form;
      p.grid = g.grid;
      p.stats_rows = g.rows;
      if (form == RDP_RING_BNRED) p.bn_rows = g.rows;
    }
    return g.fits;
  };
  const bool bn_offered = bn.bny && bn.bncoef && bn.bnpart;
  // the producer's BN + ReLU applied to the input: nothing but the ring can read a pre-BN tensor
  if (in.iscale) return !bn_offered && !wpool && !wup && ring_fused(RDP_RING_BNIN) ? p : none;
  // the owner's BN-backward rows from the ring epilogue; where it does not fit, the decision below is the one
  // without the block, and only a split-K reduce can still write the rows (rdp_conv_fuse_ok)
  if (bn_offered && ring_fused(RDP_RING_BNRED)) return p;

  // first layer (3-channel input, packed K): auto for it (IGEMM4_256 runs the packed implicit GEMM, the tests'
  // second opinion)
  if (kernel == RDP_CONV_FIRST || (autok && packed)) {
    const RdpFirstGeo g = rdp_first_geo(c, taps, packed);
    if (g.fits) {
      p.kernel = RDP_CONV_FIRST;
      p.grid = g.grid;
      p.stats_rows = g.rows;
      return p;
    }
    if (!autok) return none;
  }
  // eval (BN folded, one destination) on small maps: the row-band kernel, MaxPool2d fused
  if (kernel == RDP_CONV_ROWBAND || autok) {
    if (c.escale && c.eshift && !c.stats && !c.y2 && taps == 9 && !packed) {
      const bool pool = wpool && c.H % 2 == 0 && c.W % 2 == 0;
      const long pbytes = pool ? rdp_conv_pool_bytes(c, fuse) : 0;
      auto take = [&](const RdpConv& cw, int mode) {
        const RdpRowbandGeo g = rdp_rowband_geo(cw, pool, pbytes, fuse.ppitch, mode);
        if (!g.fits) return false;
        p.kernel = RDP_CONV_ROWBAND;
        p.rowband_mode = mode;
        p.grid = g.grid;
        p.pool_fused = g.pools;
        return true;
      };
      // with the fragment-major weight copy: wherever its traffic model picks the kernel
      const int mode = autok && wfrag_bytes > 0 ? rdp_rowband_frag_mode(c.N, c.H, c.W, c.C1, c.C2, c.Cout) : 0;
      if (mode > 0) {
        RdpConv cf = c;
        cf.wbytes = wfrag_bytes;
        cf.ldw = 0;
        if (take(cf, mode)) return p;
      }
      if ((!autok || rdp_rowband_auto(c.N, c.H, c.W, Cin, c.Cout, wpool)) && take(c, 0)) return p;
    }
    if (!autok) return none;
  }
  // row ring: 64 -> 64 / 128 channels, 3x3, one source. Auto only when its grid (one block per pair of 64-pixel
  // row segments, <= 256) fills the chip: at N = 1, 128^2 x 64 -> 128 the 128-block ring took 15.2 us vs 11.9 us
  // for the implicit GEMM
  const long ring_pairs = c.W % 64 == 0 ? (long)c.N * (c.W / 64) * c.H / 2 : 0;
  if (kernel == RDP_CONV_RING || (autok && ring_pairs >= 256)) {
    if (taps == 9 && !packed && c.C2 == 0 && c.x2 == nullptr) {
      RdpRingGeo g;
      if (wpool && !c.stats && !c.y2 && c.escale)  // eval: MaxPool2d fused into the ring epilogue
        g = rdp_ring_geo(c, RDP_RING_POOL, fuse.ppitch, 256);
      const bool pools = g.fits;
      if (!pools) g = rdp_ring_geo(c, RDP_RING_PLAIN, 0, 256);
      if (g.fits) {
        p.kernel = RDP_CONV_RING;
        p.ring_form = pools ? RDP_RING_POOL : RDP_RING_PLAIN;
        p.pool_fused = pools;
        p.grid = g.grid;
        p.stats_rows = g.rows;
        return p;
      }
    }
    if (!autok) return none;
  }
  // two-source row ring: 128 input channels -> 64, 3x3, one destination; 128 -> 128 as two launches over the
  // output-channel halves (each reads the input)
  {
    const bool two = c.C1 == 64 && c.C2 == 64 && c.x2 != nullptr;
    const bool one = c.C1 == 128 && c.C2 == 0 && c.x2 == nullptr;
    const bool c64 = c.Cout == 64 && (kernel == RDP_CONV_RING2 || (autok && ring_pairs >= 256));
    const bool c128 = c.Cout == 128 && (kernel == RDP_CONV_RING2X2 || (autok && ring_pairs >= RDP_RING2_X2_PAIRS));
    if ((c64 || c128) && taps == 9 && !packed && (two || one) && c.y2 == nullptr && !wpool && !wup) {
      const RdpRingGeo g = rdp_ring2_geo(rdp_ring2_sources(c), 256, c.Cout, 0);
      if (g.fits) {
        p.kernel = c64 ? RDP_CONV_RING2 : RDP_CONV_RING2X2;
        p.launches = c.Cout / 64;
        p.grid = g.grid;
        p.stats_rows = g.rows;
        return p;
      }
    }
    if (kernel == RDP_CONV_RING2 || kernel == RDP_CONV_RING2X2) return none;
  }
  {
    const RdpHaloGeo g = rdp_halo_geo(c, taps, packed);
    // auto: the halo kernel wins only where a 64-channel output reads >= 256 input channels
    // (measured, scripts/conv_microbench.py); elsewhere the implicit GEMM's 2 blocks/CU overlap better
    const bool halo_auto = autok && g.ntiles >= 256 && c.Cout == 64 && Cin >= 256;
    if (g.shape && (kernel == RDP_CONV_HALO || halo_auto)) {
      if (!g.fits) return none;
      p.kernel = RDP_CONV_HALO;
      p.grid = g.grid;
      p.stats_rows = g.rows;
      return p;
    }
    if (kernel == RDP_CONV_HALO) return none;
  }
  // ---- the implicit GEMM and ping-pong kernels (conv_igemm.hip)
  RdpGemmShape g;
  g.M = c.N * c.H * c.W; g.Cout = c.Cout; g.Cy1 = c.Cy1; g.packed = packed; g.stats = c.stats != nullptr;
  g.N = c.N; g.uH = fuse.uH;
  if (packed) {
    if (c.C1 != 8 || c.C2 != 0 || taps != 9 || c.ldw != 128) return none;
    g.nks = 2;
  } else {
    if (c.C1 % 64 || c.C2 % 64 || (taps != 9 && taps != 1)) return none;
    g.nks = taps * (Cin / 64);
    if (c.ldw < taps * Cin) return none;
  }
  if (c.Cout % 64 || c.Cy1 % 8) return none;  // widened 16-B epilogue stores never straddle the split
  if (c.xbytes1 >= kMaxBytes || c.xbytes2 >= kMaxBytes || c.ybytes1 >= kMaxBytes || c.ybytes2 >= kMaxBytes)
    return none;
  const long wse = rdp_conv_ws_limit(has_ws, ws_elems);
  const RdpConvFuseOk ok = rdp_conv_fuse_ok(c, fuse, want_fused, bn);
  int k = kernel;
  if (autok && !packed) {
    // the ping-pong 256 x 256 kernel wherever its tile grid fills the chip (>= 256 tiles of 256 pixels x 256
    // couts; fewer tiles leave CUs idle at one block per CU). Measured (scripts/conv_microbench.py, bs 64, one
    // MI355X): 64^2 256->256 903 -> 1082 TF/s, 32^2 512->512 962 -> 1205, 32^2 512+512->256 927 -> 1120; bs 64
    // step 2973 -> 3150 img/s. The 256 x 128 form is 2-4 % faster than the 128 x 128 kernel where K >= 1152
    // (128^2 128->128 851 -> 889, 64^2 256+256->128 882 -> 907; slower at K = 576) and +1.0-1.4 % on the bs 64
    // step: only where K is long enough (>= 128 input channels).
    const long tiles256 = (long)(g.M + 255) / 256 * (c.Cout / 256);
    const long tiles128 = (long)(g.M + 255) / 256 * (c.Cout / 128);
    const bool pp = c.Cy1 % 32 == 0 && c.escale == nullptr;
    if (pp && c.Cout % 256 == 0 && tiles256 >= 256) k = RDP_CONV_PP256;
    else if (pp && c.Cout % 128 == 0 && tiles128 >= 256 && Cin >= 128) k = RDP_CONV_PP128;
    // small M x long K (training): split-K ping-pong 256 x 128 where its split exists and the 128 x 128
    // kernel would split K too (measured, scripts/conv_microbench.py --batch 4 --ws 1, one MI355X: 32^2
    // 1024->512 63.5 -> 53.2 us, 512->512 39.9 -> 36.7, 512+512->256 39.0 -> 36.7, 64^2 256->128 31.5 ->
    // 29.4; where the 128 x 128 grid needs no split (64^2 256->256) the unsplit kernel wins, 32.9 vs 39.5,
    // and at M = 1024 (16^2 512->1024: 29.5 vs 31.0 us) the 128 x 128 split does)
    // (eval too, BN fold in the shared reduce: the batched serving network at N = 4, scripts/rowband_bench.py
    // --batch 4 --variants 0,7: 32^2 1024->512 63.2 -> 52.3 us, 512->512 + pool 39.3 -> 36.4)
    else if (c.Cout % 128 == 0 && c.Cy1 % 32 == 0 && Cin >= 128 && g.M >= 4096 &&
             (long)(g.M + 127) / 128 * (c.Cout / 128) < 192 && pp_split_enabled() &&
             rdp_pp_split(g.M, c.Cout, 128, g.nks, wse) > 1)
      k = RDP_CONV_PPSK128;
  }
  // the fallback: 8-wave blocks (64 x 32 per wave; twice the waves per SIMD to hide the per-step
  // barrier + DMA latency, 1.5x the LDS fragment reads per MFMA)
  // (measured dead end: 256 x 256 / 256 x 128 tiles in this 2-phase structure, one 8-wave block
  // per CU -- 49 spilled VGPRs at 256 x 256; +6 % on 32^2 x 512 -> 512 only, -5..-40 % elsewhere)
  if (k == RDP_CONV_AUTO) k = c.Cout % 128 == 0 ? RDP_CONV_IGEMM8_128 : RDP_CONV_IGEMM8_256;
  RdpIgemmGeo r;
  switch (k) {
    case RDP_CONV_PP256: p.BN = 256; break;
    case RDP_CONV_PP128: p.BN = 128; break;
    case RDP_CONV_PPSK128: p.BN = 128; break;
    case RDP_CONV_PPSK256: p.BN = 256; break;
    case RDP_CONV_IGEMM8_128: p.BM = 128; p.BN = 128; p.waves = 8; break;
    case RDP_CONV_IGEMM8_256: p.BM = 256; p.BN = 64; p.waves = 8; break;
    case RDP_CONV_IGEMM4_128: p.BM = 128; p.BN = 128; p.waves = 4; break;
    case RDP_CONV_IGEMM4_256: p.BM = 256; p.BN = 64; p.waves = 4; break;
    default: return none;
  }
  if (p.BM == 0) {  // ping-pong: 256-pixel tiles, 8 waves
    p.BM = 256;
    p.waves = 8;
    int d = 1;
    if (k == RDP_CONV_PPSK128 || k == RDP_CONV_PPSK256) {
      d = rdp_pp_split(g.M, c.Cout, p.BN, g.nks, wse);
      if (d < 2) return none;
    }
    r = rdp_pp_geo(g, p.BN, d, wse > 0, ok);
  } else {
    // 2 blocks per CU, every block resident (finer grids were measured slower: profiles/dead_ends.md)
    r = rdp_igemm_geo(g, p.BM, p.BN, wse, 512, ok);
  }
  if (!r.fits) return none;
  p.kernel = k;
  p.ksplit = r.ksplit;
  p.grid = r.grid;
  p.rgrid = r.rgrid * r.rgrid_y;
  p.stats_rows = r.rows;
  p.ws_elems = r.ksplit > 1 ? (long)r.ksplit * g.M * c.Cout : 0;
  p.pool_fused = r.pool;
  p.up_fused = r.up;
  p.bn_rows = r.bn ? r.rows : 0;
  return p;
}

// ---- sizing ----------------------------------------------------------------------------------------------------
RdpConvPlan rdp_conv_plan_dense(const RdpConvQuery& q) {
  // only the null / non-null state of the pointers and the sizes are looked at
  static char mark;
  static float fmark;
  const int Cin = q.C1 + q.C2, Cy1 = q.split > 0 ? q.split : q.Cout;
  auto bytes = [&](int C) { return (long)q.N * q.H * q.W * C * 2; };
  RdpConv c;
  c.x1 = &mark; c.C1 = q.C1; c.pitch1 = q.C1; c.xbytes1 = bytes(q.C1);
  if (q.C2) { c.x2 = &mark; c.C2 = q.C2; c.pitch2 = q.C2; c.xbytes2 = bytes(q.C2); }
  c.w = &mark; c.ldw = q.packed ? 128 : q.taps * Cin; c.wbytes = (long)q.Cout * c.ldw * 2;
  c.y1 = &mark; c.Cy1 = Cy1; c.ypitch1 = Cy1; c.ybytes1 = bytes(Cy1);
  if (q.split > 0) { c.y2 = &mark; c.ypitch2 = q.Cout - Cy1; c.ybytes2 = bytes(q.Cout - Cy1); }
  c.N = q.N; c.H = q.H; c.W = q.W; c.Cout = q.Cout;
  if (q.stats) c.stats = &fmark;
  if (q.eval) { c.escale = &fmark; c.eshift = &fmark; c.erelu = 1; }
  RdpConvFuse fuse;
  if (q.pool) { fuse.pool = &mark; fuse.ppitch = q.Cout; }
  if (q.up) { fuse.up = &mark; fuse.upitch = q.Cout; fuse.uH = 2 * q.H; fuse.uW = 2 * q.W; }
  RdpConvBnBwd bn;
  if (q.bn) { bn.bny = &mark; bn.bnypitch = q.Cout; bn.bncoef = &fmark; bn.bnpart = &fmark; }
  RdpConvBnIn in;
  if (q.bnin) { in.iscale = in.ishift = &fmark; in.aout = &mark; in.apitch = q.C1; in.abytes = bytes(q.C1); }
  return rdp_conv_plan(c, q.taps, q.packed, q.kernel, q.ws_elems > 0, q.ws_elems, fuse, q.pool || q.up, bn, in,
                       q.wfrag ? (long)q.Cout * 9 * Cin * 2 : 0);
}

long rdp_conv_ws_elems(int N, int H, int W, int C1, int C2, int Cout, int taps, int packed, int kernel) {
  RdpConvQuery q;  // the training-form conv, offered every element a split may use
  q.N = N; q.H = H; q.W = W; q.C1 = C1; q.C2 = C2; q.Cout = Cout; q.taps = taps; q.packed = packed; q.kernel = kernel;
  q.ws_elems = 1L << 29;
  return rdp_conv_plan_dense(q).ws_elems;
}

int rdp_conv_stats_rows(long M, int Cout, int kernel) {
  // forced tiles: one row per (M tile, wave row), or up to 512 rows when split-K reduces them
  if (kernel == RDP_CONV_IGEMM4_128 && Cout % 128 == 0) return (int)std::max<long>((M + 127) / 128 * 2, 512);
  if (kernel == RDP_CONV_IGEMM4_256) return (int)std::max<long>((M + 255) / 256 * 4, 512);
  // auto / halo: upper bound over every tile choice (halo: up to 8 wave rows per 256-pixel tile)
  // split-K reduce: up to 512 rows
  const long a = (M + 127) / 128 * 2, b = (M + 255) / 256 * 8;
  const long ab = a > b ? a : b;
  // + room for batch-chunked launches (conv_fwd: tensors past 2 GiB run as image slices, each with
  // its own 512-row floor and tile rounding): one chunk per 2 GiB of a 1024-channel bf16 tensor
  const long chunks = 1 + M * 2048 / (1L << 31);
  return (int)((ab > 512 ? ab : 512) + 520 * chunks);
}
