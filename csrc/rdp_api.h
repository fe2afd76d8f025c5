// The GPU launchers (rdp_*) and their sizing helpers: the one declaration of each, included by the .hip file
// that defines it and by every caller (csrc/bindings.cpp, csrc/serve_runtime.cpp, the conv dispatcher), so the
// compiler compares definition and use. Every launcher enqueues on the given stream and returns without waiting.
#pragma once
#include <hip/hip_runtime_api.h>

#include "rdp_host_api.h"

// The conv family's operand blocks (RdpConv, RdpConvFuse, RdpConvBnBwd, RdpConvBnIn, RdpRingHead, RdpWgrad, RdpWgradBn,
// RdpUpT), the
// kernel names and the plans
#include "conv_plan.h"

extern "C" {

// ---- csrc/comm.hip --------------------------------------------------------------------------------------------
int rdp_comm_emulate(double us, int blocks, hipStream_t s);
// scratch: >= 2 * traffic_bytes (16-byte aligned); traffic_bytes: bytes read (and as many written)
int rdp_comm_emulate_traffic(double us, int blocks, void* scratch, long scratch_bytes, long traffic_bytes,
                             hipStream_t s);

// ---- csrc/conv_first.hip --------------------------------------------------------------------------------------
// Returns the number of stats rows written (training) / 0, or -1 if the conv is not this kernel's (rdp_first_geo).
int rdp_conv_first(const RdpConv& c, hipStream_t s);

// ---- csrc/conv_halo.hip ---------------------------------------------------------------------------------------
// Returns stats rows written (>= 0) or -1 if unsupported (rdp_halo_geo).
int rdp_conv_halo(const RdpConv& c, hipStream_t s);

// ---- csrc/conv_igemm.hip --------------------------------------------------------------------------------------
// ConvTranspose2d(k=2, s=2) + bias straight into its (padded) output map u [N][t.H2][t.W2][ypitch1]: the
// 1x1 GEMM yT[px][sub * C + c] = sum_ci x[px][ci] Wt[sub * C + c][ci] on the ping-pong kernel with the
// sub-pixel scatter + bias in its epilogue (no yT round trip and no upT_shuffle pass). c: x1 = x, w = Wt,
// y1 = u, Cout = 4C, N / H / W = the low-res map (rdp_upT_fwd_geo). u's border outside the 2h x 2w window at
// (t.oy, t.ox) is not written (the caller zeroes it once). Returns 0, or -1 where the ping-pong grid would not
// fill the chip / the shape does not fit (the caller then runs the GEMM + upT_shuffle).
int rdp_conv_upT_fwd(const RdpConv& c, const RdpUpT& t, const float* bias, hipStream_t s);
// ConvTranspose2d(k=2, s=2) input gradient straight from the output gradient du [N][t.H2][t.W2][C] (the
// window 2h x 2w at (t.oy, t.ox)): dx[px][ci] = sum_(sub, c) du[sub-pixel sub of px][c] Wd[ci][sub * C + c]
// on the ping-pong kernel, its A operand DMA'd from the 4 sub-pixels as 4 "taps" (no unshuffled copy
// of du). c: x1 = du, w = the [Cin][4C] dgrad weight, y1 = dx, Cout = Cin, N / H / W = the low-res map
// (rdp_upT_dgrad_geo). Returns 0, or -1 where the ping-pong grid would not fill the chip / the shape does not
// fit (the caller unshuffles and runs the 1x1 GEMM).
int rdp_conv_upT_dgrad(const RdpConv& c, const RdpUpT& t, hipStream_t s);
// The conv dispatcher: launches what rdp_conv_plan (conv_plan.h) picks. Returns the number of stats-slab rows
// written, or -1 (nothing launched) where the plan is unsupported. kernel: RDP_CONV_AUTO, or the RdpConvKernel to
// force. ws: the split-K fp32 slab of ws_elems elements (rdp_conv_ws_elems), or nullptr. wfrag / wfrag_bytes: the
// fragment-major copy of the weights for the row-band kernel, or nullptr. *pooled = 1 if fuse's pool / upsample was
// written, else 0 (the caller launches the pool / upsample; nullptr: no fusion). *bnrows = the rows written to
// bn.bnpart by the ring epilogue or the split-K reduce, else 0 (the caller runs bn_relu_bwd_reduce). in: x1 is
// the producer's pre-BN output (only the ring's BNIN form runs it: anything else is unsupported).
int rdp_conv_igemm(const RdpConv& c, int taps, int packed, int kernel, float* ws, long ws_elems, const void* wfrag,
                   long wfrag_bytes, const RdpConvFuse& fuse, int* pooled, const RdpConvBnBwd& bn, int* bnrows,
                   const RdpConvBnIn& in, hipStream_t s);

// ---- csrc/conv_ring.hip ---------------------------------------------------------------------------------------
// The ring kernel (3x3, one 64-channel source, 64 or 128 outputs -- split at a multiple of 32 into two
// destinations --, W % 64 == 0, even H: rdp_ring_geo) in the RdpRingForm the plan names: PLAIN, POOL (eval, 64 ->
// 64: also MaxPool2d(2) of the output into fuse.pool), BNRED (the owner layer's BN-backward partial rows into
// bn.bnpart) or BNIN (in: the producer's BN + ReLU applied to the staged input). Returns the partial rows it
// writes, or -1 (nothing launched) when the form does not apply.
int rdp_conv_ring(const RdpConv& c, int form, const RdpConvFuse& fuse, const RdpConvBnBwd& bn, const RdpConvBnIn& in,
                  hipStream_t s);
// Eval conv (64 -> 64, BN folded + ReLU; c has no destination) fused with the serving 1x1 head: writes only the u8
// mask of the 64-channel output. h.K = 1: logit > h.thr; 2 <= h.K <= 8: arg-max class == h.cls (ties to the lowest
// class), bit for bit the mask rdp_headk_mask writes from the stored output. Returns 0, or -1 (nothing launched)
// where the ring kernel does not apply and, for K classes, where the input is a strided view (pitch != 64) or K /
// cls are out of range.
int rdp_conv_ring_head(const RdpConv& c, const RdpRingHead& h, hipStream_t s);
// Two-source row ring (see conv_ring2_kernel): x1 / x2 = the two 64-channel sources (for one
// 128-channel tensor: its two halves), 64 outputs into y1, 3x3, W % 64 == 0, even H. cout_total / co0: the
// launch computes output channels co0 .. co0 + 63 of a cout_total-channel conv (w, y1, escale / eshift
// already offset by the caller; the stats rows are [rows][2][cout_total], this launch's 64 columns
// at co0). Returns the stats rows written (grid * 4), or -1 when not applicable.
int rdp_conv_ring2(const RdpConv& c, int max_blocks, int cout_total, int co0, hipStream_t s);

// ---- csrc/conv_rowband.hip ------------------------------------------------------------------------------------
// Eval conv on the row-band kernel into y1; pool (optional, pbytes / ppitch): MaxPool2d(2) of the output where the
// kernel can fuse it. Returns 1 if it also wrote the pool, 0 if not, < 0 (nothing launched) when the shape does
// not fit. wfrag 1: w is the fragment-major copy of the OHWI weights instead of OHWI; 2: that copy on the
// activation-staged kernel (rdp_rowband_frag_mode picks).
int rdp_conv_rowband_ex(const RdpConv& c, void* pool, long pbytes, int ppitch, int wfrag, hipStream_t s);
// The chain launch: layer 0 reads x (C0 channels), layer l > 0 reads layer l - 1's output; every layer is
// an eval conv (BN folded + ReLU) on the same N x H x W map. cnt: >= 1 + nl * N * H ints, err: 1 int.
// Returns 0, or < 0 (nothing launched) when a layer does not fit the row-band kernel.
int rdp_conv_rowband_chain(int nl, const void* x, long xbytes, int C0, int xpitch, const void* const* w,
                           const long* wbytes, const int* ldw, void* const* y, const long* ybytes,
                           const int* ypitch, const int* cout, const float* const* escale,
                           const float* const* eshift, int N, int H, int W, int* cnt, int* err, hipStream_t s);

// ---- csrc/conv_wgrad.hip --------------------------------------------------------------------------------------
// Each launches what rdp_wgrad_plan (conv_plan.h) says, then the slab reduce into g.out, and returns the split
// count, or an RdpWgradStatus < 0 (nothing launched). Slab sizing: rdp_conv_wgrad_slab_elems and
// rdp_conv_wgrad_halo_slab_elems, declared with the plan.
// kernel: RDP_WGRAD_AUTO, GENERIC or HALO; splits: asked of the generic kernels (the halo / ring kernels choose)
int rdp_conv_wgrad(const RdpWgrad& g, int kernel, int splits, hipStream_t s);
// ConvTranspose2d(k=2, s=2) weight gradient straight from its output gradient du [N][t.H2][t.W2][C] (the
// window 2h x 2w at (t.oy, t.ox)) and its input x [N][h][w][Cin]: out[ci][(sub, c)] (+)= sum_px
// x[px][ci] du[sub-pixel sub of px][c] -- the generic kernel's role-swapped GEMM (columns = the 4
// sub-pixels x C, "couts" = Cin) reading du at the sub-pixels instead of an unshuffled copy.
// g: x1 = du (C1 = C), dy = x, Cout = Cin, taps = 4, N / H / W = the low-res map.
int rdp_conv_wgrad_upT(const RdpWgrad& g, const RdpUpT& t, int splits, hipStream_t s);
// The first layer with its BN backward applied on the fly. g: x1 = the packed 8-channel input, no dy.
int rdp_wgrad_first_bn(const RdpWgrad& g, const RdpWgradBn& bn, int splits, hipStream_t s);
// The two-level reduce of a planned weight gradient's slab g.slab into g.out (p.reduce)
void rdp_wgrad_reduce(const RdpWgrad& g, const RdpWgradPlan& p, hipStream_t s);

// ---- csrc/data_kernels.hip ------------------------------------------------------------------------------------
// exactly one of tgt_f (one-class: fp32 mask value) / tgt_u (K-class: u8 id, 255 outside the frame) is set
int rdp_batch_augment(const void* x, const void* y, const int* idx, const float* params, int S, int N, int H, int W,
                      void* x_out, float* tgt_f, void* tgt_u, hipStream_t s);
int rdp_area_maxtap();
int rdp_resize_area_u8(const void* in, int h, int w, int C, const int* ys, const int* yn, const double* yw,
                       const int* xs, const int* xn, const double* xw, int H, int W, int swap_rb, void* out,
                       hipStream_t s);

// ---- csrc/geo_spline.hip --------------------------------------------------------------------------------------
int rdp_geo_spline_res_len(int nsamp);
// rdp_geo_spline (presorted, serving) for n <= 4 frames in one launch: per-frame arrays of its buffers
int rdp_geo_spline_batch(int n, int nbins, int kcap, const int* const* kout, const int* const* npts,
                         double* const* sorted, double* const* u, int ecap, double s, int k, int nsamp, double eps,
                         int min_points, int min_edge, const int* const* cov, int ncov, double* const* res,
                         const void* const* mask, void* const* mask_host, long mask_bytes, hipStream_t st);
// sort the per-bin edge points (out [nbins][kcap][4], kout) into sorted [ecap][3] and fit/evaluate.
int rdp_geo_spline(const double* out, int nbins, int kcap, const int* kout, const int* npts, double* sorted,
                   int* gperm, double* u, int ecap, double s, int k, int nsamp, double eps, int min_points,
                   int min_edge, const int* cov, int ncov, double* res, double* dbg, int presorted,
                   const void* mask, void* mask_host, long mask_bytes, hipStream_t st);

// ---- csrc/geometry.hip ----------------------------------------------------------------------------------------
int rdp_geo_nblocks(int H);
// int32 workspace needed beyond the per-row-block counts: bin_of + bidx [cap] each + 2 x 128
long rdp_geo_work_ints(int H, int W);
// work_i: [nblk] counts | [cap] bin_of | [cap] bidx | [128] cnt | [128] cursor ; work_d: xmin/xmax
// pts [cap][4]; out [nbins][kcap][4]
// m256 != nullptr (serving form): `mask` is an OUTPUT, derived from the mh x mw model mask by
// nearest upsampling, and cov[nblk] receives per-row-block coverage counts. edges == nullptr: no
// packed edge list (the on-device spline reads the per-bin slabs directly). sorted != nullptr: the
// x-sorted edge points [secap][3] are written too (gperm: 2*secap ints of sort scratch), so the
// spline stage runs with presorted = 1.
int rdp_geo_edges(const void* mask, const void* depth, int H, int W, double fx, double fy, double cx, double cy,
                  double scale, int* counts, double* xmin, double* xmax, double* pts, int cap, int* npts,
                  double* out, int kcap, int* kout, int nbins, double top, int min_points, double* edges, int ecap,
                  int* hdr, const void* m256, int mh, int mw, int* cov, double* sorted, int* gperm, int secap,
                  void* mask_host, hipStream_t s);
// The serving form of rdp_geo_edges for n <= GEO_BATCH frames of one camera in ONE launch per stage
// (blockIdx.y = frame): each frame's buffers as rdp_geo_edges takes them (array of n per field). The
// stages are latency-bound small grids, so n frames cost about what one does (a batch of 4 served frames:
// 4 x 48 us of geometry as per-frame launches, profiles/serve_batch.md).
int rdp_geo_edges_batch(int n, const void* const* mask, const void* const* depth, int H, int W, double fx,
                        double fy, double cx, double cy, double scale, int* const* counts, double* const* xmin,
                        double* const* xmax, double* const* pts, int cap, int* const* npts, double* const* out,
                        int kcap, int* const* kout, int nbins, double top, int min_points, const void* const* m256,
                        int mh, int mw, int* const* cov, double* const* sorted, int* const* gperm, int secap,
                        void* const* mask_host, hipStream_t s);

// ---- csrc/head_loss.hip ---------------------------------------------------------------------------------------
int rdp_head_partial_blocks(long M);
// coef != nullptr: `a` is the last conv's pre-BN output; BN+ReLU are applied on the fly.
// gpart/bnpart != nullptr (needs coef, dice_w == 0): also the backward partials (head_fwd_kernel GRAD).
int rdp_head_fwd(const void* a, int apitch, const float* w, const float* b, const float* target, float* logits,
                 float* partial, float* sums, float* loss, int M, float dice_w, float dice_eps, const float* coef,
                 float* gpart, float* bnpart, float gscale, hipStream_t s);
// head weight / bias gradient from the [nb][65] partials of a GRAD forward
int rdp_head_grad_finalize(const float* gpart, int M, float* gw, float* gb, hipStream_t s);
// coef != nullptr: BN-fused variant (da unused; bnpart receives the BN backward partial rows).
// Returns the number of partial rows.
int rdp_head_bwd(const void* a, int apitch, const float* w, const float* logits, const float* target,
                 const float* sums, void* da, int dapitch, float* partial, float* gw, float* gb, int M,
                 float dice_w, float dice_eps, float gscale, const float* coef, float* bnpart, hipStream_t s);
int rdp_head_bn_bwd_apply(const void* y, int ypitch, const float* w, const float* logits, const float* target,
                          const float* sums, const float* coef, const float* coef2, void* dy, int dypitch, int M,
                          float dice_w, float dice_eps, float gscale, hipStream_t s);
int rdp_head_mask(const void* a, int apitch, const float* w, const float* b, float logit_thr, void* mask, int M,
                  hipStream_t s);

// ---- csrc/head_multi.hip --------------------------------------------------------------------------------------
int rdp_headk_partial_blocks(long M);
// Plain mode (cw == null and dice_w == 0): partial >= blocks * 2 floats, sums >= 2. Extended mode (class
// weights cw [K] and / or a soft Dice term, dice_w >= 0, dice_eps > 0): partial >= blocks * (2 + 3K),
// sums >= 2 + 3K = {sum cw*ce, W, I_k, P_k, T_k}. Returns the number of partial rows, < 0 if nothing was launched.
int rdp_headk_fwd(const void* a, int apitch, const float* w, const float* b, const void* labels, float* logits,
                  float* partial, float* sums, float* loss, int M, int K, const float* cw, float dice_w,
                  float dice_eps, hipStream_t s);
// partial: >= blocks * (K * 64 + K) floats; gw [K][64], gb [K]; cw / dice_w / dice_eps as given to rdp_headk_fwd
int rdp_headk_bwd(const void* a, int apitch, const float* w, const float* logits, const void* labels,
                  const float* sums, void* da, int dapitch, float* partial, float* gw, float* gb, int M, int K,
                  float gscale, const float* cw, float dice_w, float dice_eps, hipStream_t s);
int rdp_headk_mask(const void* a, int apitch, const float* w, const float* b, int cls, void* mask, int M, int K,
                   hipStream_t s);

// ---- csrc/jpeg_entropy.hip ------------------------------------------------------------------------------------
// scan: cap_bytes (a multiple of 4) of de-stuffed scan, of which *nbits (device) are the frame's; tables:
// rdp_jpeg_scan's block; geo: rdp_jpeg_meta's int32[32]; coefs: cap_coefs int16 (16-byte aligned);
// work: rdp_jpeg_entropy_work_words(cap_bytes, S) int32; status: one device-visible int32 (0 ok, 1
// corrupt). S: bits per subsequence, a multiple of 32, >= 64, 0 = the tuned default. After the launches
// work[stats_word] holds (subsequences, rounds); *stats_word (optional) receives that offset.
int rdp_jpeg_entropy_gpu(const void* scan, long cap_bytes, const int* nbits, const void* tables, const int* geo,
                         void* coefs, long cap_coefs, int* work, long work_words, int* status, int S,
                         long* stats_word, hipStream_t st);

// ---- csrc/mask_components.hip ---------------------------------------------------------------------------------
// In place on n contiguous u8 H x W masks (blockIdx.x = frame, each on its own): the 8-connected components with
// fewer than min_area pixels are zeroed and, with keep_largest, every survivor but the largest (ties: the one
// whose first pixel in row-major order comes first). stats (optional, device): per frame {components found,
// components kept, pixels kept, pixels removed}. One launch, no workspace. Returns 0, or -1 (nothing launched)
// unless n >= 1, H, W >= 1, H * W <= 65,536 and min_area >= 0.
int rdp_mask_components(void* mask, int n, int H, int W, int keep_largest, int min_area, int* stats /* [n][4] or null */,
                        hipStream_t s);

// ---- csrc/norm_act.hip ----------------------------------------------------------------------------------------
int rdp_bn_finalize(const float* stats, int T, int C, long count, const float* gamma, const float* beta,
                    float* rmean, float* rvar, long long* nbt, float momentum, float eps, float* coef, float* ws,
                    hipStream_t s);
int rdp_rows_fold(const float* buf, int T, int K, double* out, hipStream_t s);
int rdp_rows_hilo(const double* in, float* buf, int K, hipStream_t s);
int rdp_bn_eval_coef(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar, float eps,
                     float* coef, hipStream_t s);
int rdp_bn_relu_apply(const void* y, int ypitch, void* out, int opitch, const float* coef, int M, int C, int relu,
                      hipStream_t s);
// returns the number of partial rows written (T for bn_bwd_finalize)
int rdp_bn_relu_bwd_reduce(const void* da, int dapitch, const void* y, int ypitch, const float* coef, int M, int C,
                           int relu, float* partial, int max_blocks, hipStream_t s);
int rdp_bn_bwd_finalize(const float* partial, int T, int C, long count, const float* gamma, const float* coef,
                        float* dgamma, float* dbeta, float* coef2, float* ws, hipStream_t s);
int rdp_bn_relu_bwd_apply(const void* da, int dapitch, const void* y, int ypitch, const float* coef,
                          const float* coef2, void* dy, int dypitch, int M, int C, int relu, hipStream_t s);

// ---- csrc/optim.hip -------------------------------------------------------------------------------------------
// inc = 0: the caller advances the step counter later on this stream (rdp_wprep with step)
// g_bf16: g is bf16 (u16) instead of fp32
// max_blocks > 0 caps the grid (grid-stride loop): the overlapped update on the side stream leaves CUs to
// the next forward's first layers
int rdp_adam(float* p, const void* g, int g_bf16, float* m, float* v, void* shadow, long n, float lr, float b1,
             float b2, float eps, float wd, float gscale, int* step, int inc, int max_blocks, hipStream_t s);
// rdp_adam with the step's device scalars: g is scaled by gscale * ctl[0] (the clip coefficient) and the rate
// is lr * ctl[1] (the schedule's multiplier), both read from the 4-float block rdp_optim_ctl wrote
int rdp_adam_ctl(float* p, const void* g, int g_bf16, float* m, float* v, void* shadow, long n, float lr, float b1,
                 float b2, float eps, float wd, float gscale, int* step, const float* ctl, int inc, int max_blocks,
                 hipStream_t s);
// sum of squares of g (fp32, or bf16 with g_bf16) as one fp64 partial per block: returns the number of blocks
// written (partial[0 .. blocks)), at most rdp_grad_sqnorm_blocks(n), or max_blocks when that is smaller and
// > 0; -1 unless n > 0 and n % 4 == 0. No atomics: the same grid gives the same bits every run
int rdp_grad_sqnorm(const void* g, int g_bf16, long n, double* partial, int max_blocks, hipStream_t s);
int rdp_grad_sqnorm_blocks(long n);
// one block: ctl = {coef, mult, norm, (float)step[0]} from the partials (nblocks == 0: no norm, coef 1) and the
// device step counter; sched 0 = constant, 1 = cosine; formed in fp64, rounded once. -1 on a bad argument
int rdp_optim_ctl(const double* partial, int nblocks, double gscale, double clip, int sched, int W, int T, double r,
                  const int* step, float* ctl, hipStream_t s);
int rdp_cast_bf16(const float* p, void* out, long n, hipStream_t s);
// segs: device array of nseg WSeg {long src, long dst, int kind, cout, cin, taps, tile0, pad} (40 bytes
// each; tile0 = the running sum of wseg_tiles over the earlier segments); tiles = the table's total tile
// count (the caller's sum), blocks = grid cap (0: one block per tile, at most 4096)
int rdp_wprep(const float* master, void* out, const void* segs, int nseg, int* step, int tiles, int blocks,
              hipStream_t s);
int rdp_wseg_size();

// ---- csrc/pool_up.hip -----------------------------------------------------------------------------------------
int rdp_maxpool2_fwd(const void* x, int xpitch, void* out, int opitch, int N, int H, int W, int C, hipStream_t s);
int rdp_maxpool2_bwd(const void* dp, int dppitch, const void* x, int xpitch, const void* dskip, int dspitch,
                     void* dx, int dxpitch, int N, int H, int W, int C, hipStream_t s);
int rdp_bn_relu_apply_pool(const void* y, int ypitch, void* a, int apitch, void* pool, int ppitch,
                           const float* coef, int N, int H, int W, int C, hipStream_t s);
// returns the number of partial rows written (T for bn_bwd_finalize), -1 if not applicable
// x: the stored activation (pitch check only: the argmax is recomputed from y)
int rdp_maxpool2_bwd_bn_reduce(const void* dp, int dppitch, const void* x, int xpitch, const void* dskip,
                               int dspitch, void* dx, int dxpitch, const void* y, int ypitch, const float* coef,
                               int N, int H, int W, int C, float* partial, int max_blocks, hipStream_t s);
int rdp_upsample2_fwd(const void* x, int xpitch, void* out, int opitch, int N, int hin, int win, int Hout, int Wout,
                      int oy, int ox, int C, const float* coef, hipStream_t s);
// y/coef/partial given: fused BN-backward reduction of dx's consumer BN; returns the partial rows
// written (<= max_blocks). Otherwise returns 0.
int rdp_upsample2_bwd(const void* dout, int dpitch, void* dx, int xpitch, int N, int hin, int win, int Hout,
                      int Wout, int oy, int ox, int C, const void* y, int ypitch, const float* coef, float* partial,
                      int max_blocks, hipStream_t s);
int rdp_upT_shuffle(const void* yT, int ypitch, const float* bias, void* u, int upitch, int N, int h, int w, int H2,
                    int W2, int oy, int ox, int C, hipStream_t s);
int rdp_upT_unshuffle(const void* du, int dpitch, void* dyT, int ypitch, int N, int h, int w, int H2, int W2,
                      int oy, int ox, int C, hipStream_t s);
// partial must hold >= 1024 * K + 2 * FOLD_RB * K / groups floats
int rdp_colsum_bf16(const void* x, int pitch, long M, int K, int groups, float* partial, float* out, int accumulate,
                    hipStream_t s);

// ---- csrc/seg_metrics.hip -------------------------------------------------------------------------------------
// pixels of one block and pass: M above blocks * this takes more than one pass of the grid-stride loop
int rdp_seg_confusion_block_pixels();
// blocks of one launch over M pixels
int rdp_seg_confusion_blocks(long M);
// counts: int64 [KC * KC + 1], added to. max_blocks > 0 caps the grid (a test hook: a small M then
// takes several passes of the grid-stride loop). Returns the blocks launched, < 0 if nothing was.
int rdp_seg_confusion(const float* logits, const void* target, void* counts, long M, int K, float thr,
                      int max_blocks, hipStream_t s);

// ---- csrc/serve_kernels.hip -----------------------------------------------------------------------------------
int rdp_preprocess(const void* bgr, int H, int W, const int* ystart, const int* ysize, const float* yw,
                   const int* xstart, const int* xsize, const float* xw, int OH, int OW, int rgb, void* out,
                   hipStream_t s);
int rdp_preprocess_batch(int n, const void* const* bgr, int H, int W, const int* ystart, const int* ysize,
                         const float* yw, const int* xstart, const int* xsize, const float* xw, int OH, int OW,
                         int rgb, void* const* out, hipStream_t s);
int rdp_mask_upsample(const void* m, int mh, int mw, void* out, int H, int W, unsigned* count, hipStream_t s);
// the JPEG pixel stage of n <= 4 frames (each its coefficient / meta / planes / RGB buffers) in 2 launches
int rdp_jpeg_gpu_batch(int n, const void* const* coefs, const int* const* geo, const int* const* qt,
                       void* const* planes, int H, int W, int max_blocks, void* const* rgb, hipStream_t s);
// coefficient / plane capacity for frames of H x W (any supported sampling: Y and chroma planes at most
// MCU-padded to 16 x 16)
long rdp_jpeg_max_coefs(int H, int W);
long rdp_jpeg_plane_bytes(int H, int W);
int rdp_jpeg_gpu(const void* coefs, const int* geo, const int* qt, void* planes, int H, int W, int max_blocks,
                 void* rgb, hipStream_t s);
int rdp_h2d_copy(const void* src, void* dst, long bytes, hipStream_t s);
// n <= 16 segments, every src / dst 16-byte aligned (returns -1, nothing launched, otherwise)
int rdp_h2d_copy_multi(const void* const* src, void* const* dst, const long* bytes, int n, hipStream_t s);

}  // extern "C"
