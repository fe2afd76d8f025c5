// Host-only native entry points (csrc/jpeg.cpp, csrc/codecs.cpp, csrc/spline.cpp): the one declaration of each,
// included by the file that defines it and by every caller, so the compiler compares them. Plain C++ with no
// ROCm dependency: the stand-alone sanitizer programs under tests/native/ build against this header with g++.
#pragma once
#include <stdint.h>

extern "C" {

// ---- csrc/codecs.cpp ------------------------------------------------------------------------------------------
// width, height, bit depth of a supported PNG; returns 0, -1 (not PNG / corrupt) or -2 (unsupported)
int rdp_png_info(const uint8_t* d, long n, int* w, int* h, int* bd);
// decode into out (h * w * bd/8 bytes; 16-bit samples native-endian). 0 ok, -1 corrupt, -2 unsupported.
// `parallel`: use an rdPs band index if the file has one.
int rdp_png_decode(const uint8_t* d, long n, uint8_t* out, long out_bytes, int parallel);
// Grayscale PNG of img (h x w, row-major; bpp 1 = u8, 2 = native-endian u16), filter type 0 per row,
// deflated at `level` in `bands` row bands (> 1: the banded stream + rdPs index described above, the
// bands compressed in parallel). Returns the encoded size, or -1 if cap is too small / zlib failed.
long rdp_png_encode_gray(const uint8_t* img, int w, int h, int bpp, int level, int bands, uint8_t* out, long cap);
long rdp_png_encode_bound(int w, int h, int bpp, int bands);

// ---- csrc/jpeg.cpp --------------------------------------------------------------------------------------------
// Header summary. info (int[24]): width, height, ncomp, hmax, vmax, mcux, mcuy, restart, segments,
// then per component (3 x 5): h, v, bw, bh, tq. Returns the coefficient count, or -1 corrupt / -2
// unsupported.
long rdp_jpeg_info(const uint8_t* d, long n, int* info);
// The pixel stage's geometry block (meta int32[32]: W, H, ncomp, hmax, vmax, total blocks; per component
// c at 8 + 8c: h, v, blocks per line, block rows, first block, plane byte offset, downsampled width,
// height) from rdp_jpeg_info's header summary `hi`.
void rdp_jpeg_meta(const int* hi, int* g);
// Entropy-decode into `coefs` (rdp_jpeg_info's count, int16, plane after plane, blocks row-major,
// natural order, quantized) and the component quantisation tables into qt[3][64] (natural order).
// Restart segments are decoded in parallel when `parallel`. 0 ok, -1 corrupt, -2 unsupported.
int rdp_jpeg_decode(const uint8_t* d, long n, int16_t* coefs, long ncoefs, uint16_t* qt, int parallel);
long rdp_jpeg_tables_bytes();
long rdp_jpeg_entropy_work_words(long cap_bytes, int S);
// Upper bound of rdp_jpeg_scan's output for this stream (its entropy-coded bytes, rounded up to whole
// 32-bit words), or parse()'s error.
long rdp_jpeg_scan_bound(const uint8_t* d, long n);
// Front end of the GPU entropy decoder: what rdp_jpeg_decode accepts, without restart markers. meta
// (int32[224]: rdp_jpeg_meta's geometry, then the three quantisation tables), the packed Huffman tables
// (rdp_jpeg_tables_bytes()), and the scan bytes with the 0xFF00 stuffing removed, cut at the first marker,
// into scan[cap] (cap a multiple of 4); *nbits = 8 x the bytes written. No entropy work. 0 ok, -1 corrupt,
// -2 unsupported here (restart markers, more than two tables of a class, a scan above `cap`): the
// host decoder runs.
int rdp_jpeg_scan(const uint8_t* d, long n, int* meta, uint8_t* tables, uint8_t* scan, long cap, int* nbits);
// The GPU decoder's stages (jpeg_entropy.hip) as plain loops over the same per-lane code, workgroup by
// workgroup and round by round, so results and statistics equal the kernels'. scan[cap_bytes] (a multiple
// of 4, 4-byte aligned), S bits per subsequence (0: the default). *status: 0 ok, 1 corrupt (whenever
// rdp_jpeg_decode returns -1); stats (optional): subsequences, rounds. Returns -1 on bad arguments.
int rdp_jpeg_entropy_emulate(const uint8_t* scan, long cap_bytes, int nbits, const uint8_t* tables, const int* geo,
                             int16_t* coefs, long cap_coefs, int S, int* status, int* stats);

// ---- csrc/spline.cpp ------------------------------------------------------------------------------------------
// FITPACK fppara for iopt = 0, unit weights, ub = u[0], ue = u[m-1].
//   x: m points x idim (point-major); t: >= nest knots; c: >= nest*idim coefficients (dim-major,
//   stride nest). Returns ier (-2 polynomial, 0 ok, 1..3 FITPACK warnings, 10 invalid input).
int rdp_parcur(int idim, int m, const double* u_in, const double* x_in, double s, int k, int nest, double* t_out,
               double* c_out, int* n_out, double* fp_out);
// value / derivatives (der <= k) of a B-spline (t: n knots, c: n-k-1 coefficients) at x,
// extrapolating outside [t_k, t_{n-k-1}] like FITPACK splev(ext=0).
double rdp_splev1(const double* t, int n, const double* c, int k, double x, int der);
// Full post-edge pipeline: chord-length u, parcur(s, k), 100-sample curvature + points.
//   pts: m x 3 (sorted by x); out_pts: nsamp x 3; out: [mean_k, max_k, fp, n]; returns ier
//   (-2/0/1/2/3 like FITPACK, 10 = invalid input -> caller returns the empty result).
int rdp_fit_curvature(const double* pts, int m, double s, int k, int nsamp, double eps, double* out_pts,
                      double* out);

}  // extern "C"
