// Which conv kernel runs where: the one place that knows. Plain C++17, no HIP header: the conv family's operand
// blocks, the kernel names, one predicate + geometry function per kernel family, and rdp_conv_plan, which picks
// the kernel for a conv and says what its launch will look like. The launchers (csrc/conv_*.hip) call the same
// family functions the plan used, then fill their argument struct once and launch; sizing (workspace, stats
// rows) is asked of the plan, never re-derived. The weight gradients (RdpWgrad, rdp_wgrad_plan) and the
// ConvTranspose2d launchers' geometry follow the conv plan below. tests/test_conv_plan_cpu.py and
// tests/test_wgrad_plan_cpu.py drive this file without a GPU.
#pragma once

// ---- the conv family's operand blocks ----------------------------------------------------------------------------
// Activations are NHWC bf16 views: pointer, extent in bytes (the kernels size their buffer descriptors from it;
// every extent must stay below 2 GiB), channels and pixel pitch in elements. Every field defaults to zero / null;
// a launcher ignores the fields its kernel has no use for. The blocks hold values only: a launch that is recorded
// for replay keeps a copy. Host cells a launch writes its result to (int*) are separate parameters. The plan
// functions only test the pointers for null.
struct RdpConv {
  // the sources: the conv reads cat(x1, x2) along channels (one source: x2 = nullptr, C2 = 0)
  const void* x1 = nullptr;
  const void* x2 = nullptr;
  long xbytes1 = 0, xbytes2 = 0;
  int C1 = 0, C2 = 0, pitch1 = 0, pitch2 = 0;
  // the weights, bf16 [Cout][ldw]
  const void* w = nullptr;
  long wbytes = 0;
  int ldw = 0;
  // the destinations: output channels [0, Cy1) go to y1, [Cy1, Cout) to y2 (one destination: y2 = nullptr)
  void* y1 = nullptr;
  void* y2 = nullptr;
  long ybytes1 = 0, ybytes2 = 0;
  int Cy1 = 0, ypitch1 = 0, ypitch2 = 0;
  float* stats = nullptr;  // training: the BN partial (sum, sum of squares) rows, [rows][2][Cout]
  int N = 0, H = 0, W = 0, Cout = 0;
  // the eval epilogue y = acc * escale[c] + eshift[c], then ReLU if erelu (both null: none)
  const float* escale = nullptr;
  const float* eshift = nullptr;
  int erelu = 0;
};
// rdp_conv_igemm, eval, optional: MaxPool2d(2) of y1 into pool [N][H/2][W/2][Cout], or (exclusive) the bilinear
// x2 upsample of y1 into up [N][uH][uW][Cout] at (uoy, uox), fused into the conv where the chosen kernel can
struct RdpConvFuse {
  void* pool = nullptr;
  int ppitch = 0;
  void* up = nullptr;
  int upitch = 0, uH = 0, uW = 0, uoy = 0, uox = 0;
};
// rdp_conv_igemm, training dgrad into one BN + ReLU layer's activation gradient, optional: that layer's pre-BN
// output bny, its coefficients bncoef [mean|invstd|scale|shift] (ReLU applied), and bnpart, which receives its
// BN-backward partial rows where the kernel that runs can write them: the row ring's epilogue (RDP_RING_BNRED) or
// the split-K reduce. A block counts as offered when all three pointers are set.
struct RdpConvBnBwd {
  const void* bny = nullptr;
  int bnypitch = 0;
  const float* bncoef = nullptr;
  float* bnpart = nullptr;
};
// rdp_conv_igemm, training forward, optional (iscale set: offered): x1 is the producer layer's pre-BN output and the
// conv applies that layer's BN + ReLU (iscale / ishift per input channel) to the rows it stages; aout (optional)
// also receives the formed activation as a tensor. Only the row ring (RDP_RING_BNIN) can read such an input.
struct RdpConvBnIn {
  const float* iscale = nullptr;
  const float* ishift = nullptr;
  void* aout = nullptr;
  long abytes = 0;
  int apitch = 0;
};
// rdp_conv_ring_head: the serving 1x1 head fused into the eval ring conv, which then writes only the u8 mask.
// K = 1: mask = (logit > thr), hw [64], hb [1]; 2 <= K <= 8: mask = (arg-max class == cls), hw [K][64], hb [K]
struct RdpRingHead {
  const float* hw = nullptr;
  const float* hb = nullptr;
  int K = 1;
  float thr = 0.f;
  int cls = 0;
  void* mask = nullptr;
};

// ---- the kernels -------------------------------------------------------------------------------------------------
// What a caller may ask of rdp_conv_igemm (the bindings export the values as _C.CONV_<name>). A forced kernel that
// does not fit the conv is an error: it never becomes another kernel.
enum RdpConvKernel : int {
  RDP_CONV_UNSUPPORTED = -1,  // (plans only) no kernel fits
  // the dispatcher chooses, by the measured thresholds in rdp_conv_plan
  RDP_CONV_AUTO = 0,
  // conv_halo.hip: 256-pixel spatial tiles staged with their halo, 3x3, channels in 64s; auto where a 64-channel
  // output reads >= 256 input channels on a grid of >= 256 tiles
  RDP_CONV_HALO = 1,
  // conv_igemm.hip conv_igemm_kernel with 8-wave blocks (64 x 32 per wave), tile 128 x 128 (Cout % 128 == 0) and
  // 256 x 64: the auto fallback; splits K by itself when the tile grid is small and a workspace is given
  RDP_CONV_IGEMM8_128 = 2,
  RDP_CONV_IGEMM8_256 = 3,
  // conv_pp_kernel, the ping-pong 256 x 256 / 256 x 128 tile, one block per CU: auto (training) where its tile
  // grid fills the chip
  RDP_CONV_PP256 = 4,
  RDP_CONV_PP128 = 5,
  // conv_ring.hip: 64 -> 64 / 128 channels, 3x3, one source, W % 64 == 0, even H; the eval MaxPool2d fused where
  // asked for; auto from 256 row pairs, and at any size in its fused training forms (RdpConvBnBwd, RdpConvBnIn)
  RDP_CONV_RING = 6,
  // the ping-pong kernel with K split over work items (rdp_pp_split) + the shared reduce, 256 x 128 / 256 x 256:
  // auto (128) for small M x long K
  RDP_CONV_PPSK128 = 7,
  RDP_CONV_PPSK256 = 8,
  // conv_first.hip: the packed 3-channel first layer (auto for it; IGEMM4_256 runs the packed implicit GEMM)
  RDP_CONV_FIRST = 13,
  // conv_ring2_kernel: 128 input channels (two 64-channel sources, or one 128-channel tensor as its halves) -> 64;
  // RING2X2: 128 -> 128 as two such launches over the output-channel halves (auto from RDP_RING2_X2_PAIRS)
  RDP_CONV_RING2 = 14,
  RDP_CONV_RING2X2 = 15,
  // conv_rowband.hip: eval convs on small maps, MaxPool2d fused where the kernel can; auto by its traffic models
  // (OHWI weights: rdp_rowband_auto, fragment-major copy: rdp_rowband_frag_mode)
  RDP_CONV_ROWBAND = 16,
  // conv_igemm_kernel with 4-wave blocks (64 x 64 per wave), tile 128 x 128 (Cout % 128 == 0) and 256 x 64
  RDP_CONV_IGEMM4_128 = 128,
  RDP_CONV_IGEMM4_256 = 256,
};
struct RdpConvKernelName {
  int kernel;
  const char* name;
};
extern const RdpConvKernelName rdp_conv_kernel_names[];  // every enumerator a caller may ask for
extern const int rdp_conv_kernel_count;
const char* rdp_conv_kernel_name(int kernel);  // "UNSUPPORTED" for anything else

// ---- per-family predicate + geometry ---------------------------------------------------------------------------
// Each returns fits (the family's whole launch predicate), the grid, and rows = what the launch reports (the BN
// partial rows it writes when the block has a stats slab).

// conv_first.hip: 3-channel input stored with pitch >= 4, 64 couts, packed [64][128] weights
struct RdpFirstGeo {
  bool fits = false;
  int nseg = 0, grid = 0, rows = 0;
};
RdpFirstGeo rdp_first_geo(const RdpConv& c, int taps, int packed);

// conv_rowband.hip. wfrag 0: OHWI weights; 1: their fragment-major copy; 2: that copy on the activation-staged
// kernel. pool: a pool destination (pbytes, ppitch) is offered; pools: the launch writes it. PB, R pick the
// kernel instantiation. RDP_ROWBAND_R2=0 keeps one-row tiles on the activation-staged kernel (A/B).
struct RdpRowbandGeo {
  bool fits = false, pools = false;
  int R = 0, bands = 0, segs = 1, PB = 0, wshift = 0, cshift = 0, T = 0, grid = 0;
};
RdpRowbandGeo rdp_rowband_geo(const RdpConv& c, bool pool, long pbytes, int ppitch, int wfrag);
// Operand bytes the row-band kernel moves from L2 (every block re-reads its weight slice; every activation is read
// once per tap and per 32-channel output slice). Measured (scripts/rowband_bench.py, N = 1, MI355X) the kernel
// runs at ~8-9 TB/s of these bytes: it beats the split-K implicit GEMM + reduce pair at <= ~150 MB (17-25 % faster
// on the 64^2 128 -> 256, 32^2 256 -> 512, 16^2 512 -> 512, 32^2 512 -> 256 and 64^2 256 -> 128 layers) and loses
// from ~225 MB up (32^2 1024 -> 512: 64 vs 27 us).
long rdp_rowband_bytes(int N, int H, int W, int Cin, int Cout, int pool);
// Auto choice with OHWI weights (<= 160 MB of those bytes; a pool the kernel cannot fuse would cost a separate
// launch). RDP_ROWBAND=0 turns both auto choices off (A/B).
bool rdp_rowband_auto(int N, int H, int W, int Cin, int Cout, bool pool);
// Auto choice with the fragment-major weight copy: the wfrag mode (0 = not the row-band kernel). C1 / C2: the two
// sources' channels. Every shape predicate of rdp_rowband_geo is checked here too; the Python executor asks this
// (binding rowband_frag_mode) which layers need a fragment-major copy. RDP_ROWBAND_X_MAXPIX bounds the
// activation-staged kernel's maps (0: off).
int rdp_rowband_frag_mode(int N, int H, int W, int C1, int C2, int Cout);

// conv_ring.hip conv_ring_kernel: one block per run of row pairs (two output rows of a 64-pixel segment each)
enum RdpRingForm { RDP_RING_PLAIN, RDP_RING_POOL, RDP_RING_BNRED, RDP_RING_BNIN, RDP_RING_HEAD };
struct RdpRingGeo {
  bool fits = false;
  int WS = 0, nrows = 0, npairs = 0, pairs_per_block = 0, grid = 0, rows = 0;
};
// ppitch: the pool's pixel pitch (POOL); max_blocks caps the grid (<= 0: 256); bn: the BNRED form's operand (its
// rows go to bn.bnpart, c.stats stays null); in: the BNIN form's
RdpRingGeo rdp_ring_geo(const RdpConv& c, RdpRingForm form, int ppitch, int max_blocks,
                        const RdpConvBnBwd& bn = RdpConvBnBwd{}, const RdpConvBnIn& in = RdpConvBnIn{});
// conv_ring2_kernel: c = the two 64-channel sources; the launch computes output channels co0 .. co0 + 63 of a
// cout_total-channel conv
RdpRingGeo rdp_ring2_geo(const RdpConv& c, int max_blocks, int cout_total, int co0);
// 128 -> 128 convs as two two-source-ring launches where the ring grid is at least this large. Measured
// (scripts/conv_microbench.py --shapes 2, one MI355X): 128^2 128 -> 128 at bs 64 330.5 vs 368.9 us for the
// 256 x 128 ping-pong kernel, but 106.8 vs 98.5 at bs 16 and 45.8 vs 28.3 at bs 4 (each launch reads the
// whole input); bs-64 step 19.43 / 19.55 vs 19.47 / 19.61 ms (interleaved).
constexpr long RDP_RING2_X2_PAIRS = 4096;

// conv_halo.hip: TC x TR pixel tiles, WM x WN waves. shape: the tiling exists (channels, taps, map size);
// fits: shape and the launch's weight / split / extent checks
struct RdpHaloGeo {
  bool shape = false, fits = false;
  int TC = 0, TR = 0, WM = 0, WN = 0, tilesH = 0, tilesW = 0, tilesN = 0, ntiles = 0, grid = 0, rows = 0;
};
RdpHaloGeo rdp_halo_geo(const RdpConv& c, int taps, int packed);

// conv_igemm.hip. What the implicit GEMM sees of a conv: M pixels x Cout, nks K steps of 64
struct RdpGemmShape {
  int M = 0, Cout = 0, Cy1 = 0, nks = 0, packed = 0;
  bool stats = false;
  int N = 0, uH = 0;  // the fused upsample's grid: images x rows of its output map
};
// what the split-K reduce may fuse (each needs the split to happen): the eval pool / upsample, the BN-backward rows
// (RDP_SPLITK_BNRED=0 takes the rows out, A/B: the caller's separate pass then; the ring form is not affected)
struct RdpConvFuseOk {
  bool pool = false, up = false, bn = false;
};
RdpConvFuseOk rdp_conv_fuse_ok(const RdpConv& c, const RdpConvFuse& fuse, bool want_fused, const RdpConvBnBwd& bn);
constexpr int RDP_UP_TY = 4, RDP_UP_CG = 16;  // the fused upsample's band: output rows x channels per block
struct RdpIgemmGeo {
  bool fits = false;
  int ksplit = 1;  // > 1: work item = (tile, split), then the reduce launch
  int nks = 0;     // K steps per work item
  int tilesN = 0, ntiles = 0, grid = 0;
  int rgrid = 0, rgrid_y = 1;  // the reduce launch (0: none)
  int rows = 0;
  bool pool = false, up = false, bn = false;  // fused into the reduce
};
// Split-K of conv_igemm_kernel when the tile grid leaves most CUs idle: the smallest divisor of the K steps that
// gives >= 256 work items with >= 4 K steps each, as long as the fp32 slab fits ws_elems (1: no split).
int rdp_choose_ksplit(int ntiles, int nks, int M, int Cout, int packed, long ws_elems);
// Split-K ping-pong for the small-M / long-K convs (reference-batch training, deep layers): the 256 x BN tile grid
// alone leaves most CUs idle, so the K steps are split over d work items (the smallest divisor of nks giving >= 256
// items, one block per CU, each >= 8 K steps) when the fp32 slab d * M * Cout fits. Returns d (0: no such plan).
// RDP_PP_SPLIT=0 takes it out of the auto choice (A/B).
int rdp_pp_split(int M, int Cout, int BN, int nks, long ws_elems);
// conv_igemm_kernel<BM, BN>: ws_elems > 0 lets it split K; max_blocks caps the persistent grid
RdpIgemmGeo rdp_igemm_geo(const RdpGemmShape& g, int BM, int BN, long ws_elems, int max_blocks, RdpConvFuseOk ok);
// conv_pp_kernel<BN>: ksplit 1 = the unsplit kernel, d > 1 = rdp_pp_split's d on a workspace of >= d * M * Cout
RdpIgemmGeo rdp_pp_geo(const RdpGemmShape& g, int BN, int ksplit, bool has_ws, RdpConvFuseOk ok);

// ---- the plan --------------------------------------------------------------------------------------------------
struct RdpConvPlan {
  int kernel = RDP_CONV_UNSUPPORTED;  // the kernel that runs (never AUTO)
  int BM = 0, BN = 0, waves = 0, ksplit = 1;  // implicit GEMM / ping-pong: tile, waves per block, K split
  int rowband_mode = 0;                       // ROWBAND: the wfrag mode
  int ring_form = RDP_RING_PLAIN;             // RING: the RdpRingForm that runs (PLAIN, POOL, BNRED or BNIN)
  int launches = 1;   // conv launches (RING2X2: 2), each of grid blocks
  int grid = 0;
  int rgrid = 0;      // blocks of the split-K reduce launch (0: none)
  int stats_rows = 0; // what rdp_conv_igemm returns: the rows of the stats slab the conv writes when it has one
  long ws_elems = 0;  // fp32 workspace elements the launch uses
  bool pool_fused = false, up_fused = false;  // fuse's pool / upsample is written by the conv
  int bn_rows = 0;    // rows written to bn.bnpart (0: none, the caller runs the separate reduce pass)
};
// The dispatcher's decision, launching nothing. kernel: an RdpConvKernel (anything else: unsupported); has_ws /
// ws_elems: the split-K workspace offered; want_fused: the caller can take a fused pool / upsample (passes the
// result cell); wfrag_bytes: extent of the fragment-major weight copy (0: none given).
// bn offered (kernel AUTO or RING): the ring in its BNRED form wherever rdp_ring_geo fits it, else the decision
// without the block, the split-K reduce writing the rows where rdp_conv_fuse_ok allows, else bn_rows = 0.
// in offered: the ring in its BNIN form wherever rdp_ring_geo fits it, else unsupported.
RdpConvPlan rdp_conv_plan(const RdpConv& c, int taps, int packed, int kernel, bool has_ws, long ws_elems,
                          const RdpConvFuse& fuse, bool want_fused, const RdpConvBnBwd& bn, const RdpConvBnIn& in,
                          long wfrag_bytes);
// the part of an offered workspace a split may use: slab bytes < 2 GiB (buffer offsets)
inline long rdp_conv_ws_limit(bool has_ws, long ws_elems) {
  return has_ws && ws_elems > 0 ? (ws_elems < (1L << 29) ? ws_elems : (1L << 29)) : 0;
}
// extent of fuse.pool for the block's N images
inline long rdp_conv_pool_bytes(const RdpConv& c, const RdpConvFuse& fuse) {
  return ((long)c.N * (c.H / 2) * (c.W / 2) - 1) * fuse.ppitch * 2 + (long)c.Cout * 2;
}
// The two 64-channel sources of the two-source ring: the block itself, or (one 128-channel tensor) its halves
RdpConv rdp_ring2_sources(const RdpConv& c);

// A conv described by its shape alone, for callers without tensors (sizing, the conv_plan binding, the CPU test):
// rdp_conv_plan on a dense block of that shape. split > 0: two destinations, split | Cout - split channels;
// stats / eval: the training / eval form; pool, up (to [2H][2W]), bn, bnin, wfrag: those operands are offered;
// ws_elems > 0: a workspace of that size is. The extents are those of dense tensors, so a shape whose tensors reach
// 2 GiB plans as unsupported: callers that run such a batch as image slices ask about one slice.
struct RdpConvQuery {
  int N = 0, H = 0, W = 0, C1 = 0, C2 = 0, Cout = 0, taps = 9, packed = 0, kernel = RDP_CONV_AUTO, split = 0;
  bool stats = false, eval = false, pool = false, up = false, bn = false, bnin = false, wfrag = false;
  long ws_elems = 0;
};
RdpConvPlan rdp_conv_plan_dense(const RdpConvQuery& q);

// ---- sizing ----------------------------------------------------------------------------------------------------
// fp32 workspace elements the plan for this shape uses when offered any (0 = no split)
long rdp_conv_ws_elems(int N, int H, int W, int C1, int C2, int Cout, int taps, int packed, int kernel);
// Rows of the stats slab a conv of M pixels may write: an upper bound over every kernel `kernel` can become,
// with room for batch-chunked launches. Allocation sizes are behaviour: tests/test_conv_plan_cpu.py holds every
// plan's stats_rows against it.
int rdp_conv_stats_rows(long M, int Cout, int kernel);

// ---- ConvTranspose2d(k=2, s=2) on the ping-pong kernel ---------------------------------------------------------
// Where the 2h x 2w window of a low-res h x w map sits in the [N][H2][W2] map it is scattered to / gathered from
struct RdpUpT {
  int H2 = 0, W2 = 0, oy = 0, ox = 0;
};
// The whole launch predicate (channel multiples, placement, extents) and the tile: the 256-wide tile where its
// grid fills the chip (>= 256 tiles of 256 pixels), else the 128-wide one on the same condition, else no fit
// and the caller takes the GEMM + shuffle path.
struct RdpUpTGeo {
  bool fits = false;
  int BN = 0, tlc = 0, grid = 0;  // tlc: log2 of the output channels C (forward)
};
// c: x1 = the input [N][h][w][Cin], w = [4C][ldw], y1 = the output map u (ypitch1), Cout = 4C, N / H / W = the
// low-res map. C a power of two in 64..512: the bias fits the kernel's 4 BN statistics words at BN = 128
RdpUpTGeo rdp_upT_fwd_geo(const RdpConv& c, const RdpUpT& t);
// c: x1 = the output gradient du [N][H2][W2][C], w = the [Cin][ldw >= 4C] dgrad weight, y1 = dx, Cout = Cin,
// N / H / W = the low-res map
RdpUpTGeo rdp_upT_dgrad_geo(const RdpConv& c, const RdpUpT& t);
// Either one for dense tensors described by their shape (the upT_plan binding, the CPU test): Cin -> C channels,
// an h x w input map
RdpUpTGeo rdp_upT_geo_dense(bool fwd, int N, int h, int w, int Cin, int C, const RdpUpT& t);

// ---- the weight gradients (conv_wgrad.hip) ---------------------------------------------------------------------
// dW[cout][tap][cin] (+)= sum over pixels of x[pixel + tap][cin] * dy[pixel][cout], x = cat(x1, x2). Every kernel
// splits the pixels over blocks that write fp32 partial results [split][Cout][row] into slab; the shared two-level
// reduce sums them into out (OHWI). Same conventions as RdpConv: values only, zero defaults, extents < 2 GiB.
struct RdpWgrad {
  const void* x1 = nullptr;
  const void* x2 = nullptr;
  long xbytes1 = 0, xbytes2 = 0;
  int C1 = 0, C2 = 0, pitch1 = 0, pitch2 = 0;
  const void* dy = nullptr;
  long dybytes = 0;
  int dypitch = 0;
  float* slab = nullptr;
  long slab_elems = 0;
  float* out = nullptr;
  int accumulate = 0;
  int N = 0, H = 0, W = 0, Cout = 0, taps = 0, packed = 0;
  int cin_real = 0;  // packed: the input channels out holds (<= 8)
};
// rdp_wgrad_first_bn: the first layer's BN backward applied on the fly instead of a stored dy. da = the gradient
// of the post-ReLU activation, y = the pre-BN output (64 channels each), coef = [mean | invstd | scale | shift],
// coef2 = [A | B | K] (bn_bwd_finalize)
struct RdpWgradBn {
  const void* da = nullptr;
  const void* y = nullptr;
  long dabytes = 0, ybytes = 0;
  int dapitch = 0, ypitch = 0;
  const float* coef = nullptr;
  const float* coef2 = nullptr;
};

// AUTO, GENERIC and HALO may be asked of rdp_conv_wgrad (the bindings export every value as _C.WGRAD_<name>); the
// others are what a plan can come out as. A forced kernel that does not fit is an error, as is any other request.
enum RdpWgradKernel : int {
  RDP_WGRAD_UNSUPPORTED = -1,
  // halo / row ring where whole 64-pixel row segments exist (3x3), the generic kernel for the rest. (A ping-pong
  // 256 x 256 implicit-GEMM wgrad was built and measured 2x slower than the halo kernel: profiles/dead_ends.md.)
  RDP_WGRAD_AUTO = 0,
  // conv_wgrad_ring_kernel<64>: only on the auto path, W % 64 == 0 and Cout % 128 != 0 (the ring at 128 output
  // channels measured neutral)
  RDP_WGRAD_RING = 1,
  RDP_WGRAD_PACKED = 2,    // conv_wgrad_kernel<PACKED>: the 3-channel first layer stored as 8 channels
  RDP_WGRAD_UPT = 3,       // conv_wgrad_kernel<false, UTR>: rdp_conv_wgrad_upT
  RDP_WGRAD_GENERIC = 4,   // conv_wgrad_kernel: any taps, channels in 64s
  // conv_wgrad_halo_kernel<BN, MULTIROW>; forced: never the ring, and maps down to W = 8 (auto: W >= 32)
  RDP_WGRAD_HALO = 5,
  RDP_WGRAD_FIRST_BN = 6,  // wgrad_first_bn_kernel: rdp_wgrad_first_bn
};
extern const RdpConvKernelName rdp_wgrad_kernel_names[];
extern const int rdp_wgrad_kernel_count;
const char* rdp_wgrad_kernel_name(int kernel);  // "UNSUPPORTED" for anything else

constexpr int RDP_WGRAD_FIRST_NCOLS = 80;  // FIRST_BN's slab row: 9 taps x 8 channels, padded to 5 MFMA fragments

// what the launchers return instead of a split count
enum RdpWgradStatus : int {
  RDP_WGRAD_OK = 0,
  RDP_WGRAD_NO_FIT = -1,      // shape / request not this launcher's (nothing launched)
  RDP_WGRAD_SLAB_SMALL = -2,  // the slab does not hold the splits (generic) / a single split (halo, ring)
  RDP_WGRAD_SLAB_2GIB = -3,   // the slab extent used would reach 2 GiB (buffer offsets)
};

// Halo / ring shape rule: whole 64-pixel segments, i.e. rows of 64s, or 64 / W whole rows per segment. The auto
// dispatch takes the multi-row form from W = 32, a forced HALO from W = 8.
bool rdp_wgrad_halo_shape(int H, int W, bool forced);
// A split of `total` units over blocks: want = the count before rounding, then per_split = ceil(total / want)
// (rounded up as the kernel needs) and splits = ceil(total / per_split), so no split is empty.
struct RdpWgradSplit {
  long want = 0;
  int splits = 0, per_split = 0;
};
// generic / packed / upT / first-BN: `splits` (>= 1) pixel ranges in multiples of 64 pixels
RdpWgradSplit rdp_wgrad_pixel_split(long M, int splits);
// halo / ring: one resident wave of blocks (2 per CU at BN = 64, 1 at BN = 128; other grid targets and a minimum
// segment count per split measured neutral) over `tiles` channel tiles, at most one split per 64-pixel segment
// and what max_splits (the slab) holds. want < 1: the slab holds no split.
RdpWgradSplit rdp_wgrad_halo_split(int nseg, int tiles, int BN, long max_splits);
// rdp_wgrad_reduce's two launches over a slab [splits][Cout][ncols_pad]: level 1 (grid1 x G blocks; grid1 = 0:
// not run) sums G groups of splits in place, level 2 (grid2 blocks, vec = 4 or 1 outputs per thread) sums the
// group rows into out. ~1000 level-1 blocks, at most 32 group rows; <= 8 splits need no level 1.
struct RdpWgradReduce {
  int G = 0, grid1 = 0, grid2 = 0, vec = 0;
};
RdpWgradReduce rdp_wgrad_reduce_geo(int splits, int Cout, int ncols_pad, int taps, int cin_pad, int cin_real);

struct RdpWgradPlan {
  int status = RDP_WGRAD_NO_FIT;
  int kernel = RDP_WGRAD_UNSUPPORTED;  // the kernel that runs (never AUTO)
  int BN = 0;                          // output channels per block
  bool multirow = false;               // halo: a 64-pixel segment spans 64 / W image rows
  int tiles = 0;                       // channel tiles; grid = tiles * splits
  int splits = 0, per_split = 0;       // per_split: pixels (generic family) or 64-pixel segments (halo, ring)
  int grid = 0, block = 0;
  int ncols = 0, ncols_pad = 0;        // (tap, cin) columns and the slab's row length
  int cin_pad = 0, cin_out = 0;        // channels per tap in the slab row / in out
  int Cout = 0, taps = 0;              // out is [Cout][taps][cin_out]
  long slab_elems = 0;                 // fp32 slab elements the launch writes and the reduce reads
  RdpWgradReduce reduce;
};
// The dispatcher's decision, launching nothing. kernel: RDP_WGRAD_AUTO / GENERIC / HALO; splits: the pixel splits
// asked of the generic family (the halo / ring kernels choose their own, within g.slab_elems). upT.H2 > 0: the
// ConvTranspose2d form (x1 = du, dy = the ConvT input, Cout = its channels, taps = 4); bn.da: the first-layer form.
RdpWgradPlan rdp_wgrad_plan(const RdpWgrad& g, int kernel, int splits, const RdpUpT& upT = RdpUpT{},
                            const RdpWgradBn& bn = RdpWgradBn{});
// The same for a dense layer described by its shape alone (sizing, the wgrad_plan binding, the CPU test)
struct RdpWgradQuery {
  int N = 0, H = 0, W = 0, C1 = 0, C2 = 0, Cout = 0, taps = 9, packed = 0, cin_real = 0;
  int kernel = RDP_WGRAD_AUTO, splits = 1;
  long slab_elems = 0;
  bool upT = false, first_bn = false;
};
RdpWgradPlan rdp_wgrad_plan_dense(const RdpWgradQuery& q);
// The executor's split request for the generic family: target_blocks over the kernel's 256-column x 64-cout tiles,
// but at least 2048 pixels per split.
int rdp_wgrad_auto_splits(int N, int H, int W, int Cin, int Cout, int taps, int packed, int target_blocks);

extern "C" {
// Slab size (elements) for the generic kernel's `splits` pixel splits. The halo / row-ring kernels choose
// their own split count, capped by the slab they are given: the training step shares one slab of the
// largest generic size, which caps the deep layers' halo wgrads at 4-15 splits (~120 blocks). That is
// deliberate: sized for a full wave of halo blocks (rdp_conv_wgrad_halo_slab_elems) the wgrads run ~1.8x
// faster alone but the step got slower -- bs 64 3,120-3,131 vs 3,160-3,181 img/s, bs 4 1,405-1,409 vs
// 1,591 (same box, 2 rounds): the side-stream wgrads then take every CU from the main stream's convs.
long rdp_conv_wgrad_slab_elems(int N, int H, int W, int Cin, int Cout, int taps, int packed, int splits);
// Slab the halo / row-ring wgrad needs for one resident wave of blocks (its own split choice
// unconstrained); 0 where the auto dispatch does not pick those kernels. (conv_microbench.py sizes with it.)
long rdp_conv_wgrad_halo_slab_elems(int N, int H, int W, int Cin, int Cout);
}
