// Host sanitizer / fuzz driver for the GPU entropy decoder's host-side code: the scan front end
// (csrc/jpeg.cpp rdp_jpeg_scan) and the per-lane decode core the HIP kernels run (csrc/jpeg_sync.h),
// through its CPU emulation (rdp_jpeg_entropy_emulate: same code, same workgroup / round structure).
// Built with -fsanitize=address,undefined by tests/test_jpeg_entropy_sanitizers_cpu.py.
//
// usage: jpeg_sync_fuzz <seed.jpg> <mutations>
//   1. the seed (a baseline JPEG without restart markers) goes through scan + emulation and must equal
//      rdp_jpeg_decode (positive control);
//   2. <mutations> deterministic mutants -- every other one with the headers left intact, so most reach
//      the entropy stage -- go through the same, with every buffer sized exactly from the header (scan
//      bytes from the stream, coefficients from the geometry): a read or write past either is the
//      sanitizer's to report. Where the front end takes the stream, the emulation's verdict must be
//      rdp_jpeg_decode's, and where both accept, so must the coefficients.
// Prints "<cases> cases, <failures> failures"; exit status 0 iff no failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../csrc/rdp_host_api.h"

namespace {

std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

struct Rng {  // xorshift64*: deterministic mutants
  uint64_t s;
  uint64_t next() {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return s * 2685821657736338717ull;
  }
  size_t below(size_t n) { return n ? (size_t)(next() % n) : 0; }
};

// mutations at or after `from` (0: anywhere, the headers included)
std::vector<uint8_t> mutate(const std::vector<uint8_t>& in, Rng& r, size_t from) {
  std::vector<uint8_t> v = in;
  const int k = 1 + (int)r.below(6);
  for (int i = 0; i < k && v.size() > from; ++i) {
    const size_t at = from + r.below(v.size() - from);
    switch (r.below(6)) {
      case 0: v[at] = (uint8_t)r.next(); break;                       // random byte
      case 1: v[at] ^= (uint8_t)(1u << r.below(8)); break;            // bit flip
      case 2: v.resize(at); break;                                    // truncation
      case 3: v.insert(v.begin() + at, 0xFF); break;                  // a marker prefix
      case 4: {                                                       // duplicated range
        const size_t len = std::min<size_t>(1 + r.below(64), v.size() - at);
        std::vector<uint8_t> seg(v.begin() + at, v.begin() + at + len);
        v.insert(v.begin() + from + r.below(v.size() - from), seg.begin(), seg.end());
        break;
      }
      default: v.erase(v.begin() + at, v.begin() + std::min(v.size(), at + 1 + r.below(16))); break;
    }
  }
  return v;
}

long g_cases = 0, g_fail = 0, g_scanned = 0, g_equal = 0, g_corrupt = 0;

void fail(const char* what, long i) {
  ++g_fail;
  std::printf("FAIL %s (case %ld)\n", what, i);
}

size_t scan_begin(const std::vector<uint8_t>& v) {  // first byte after the SOS header
  for (size_t i = 2; i + 3 < v.size(); ++i)
    if (v[i] == 0xFF && v[i + 1] == 0xDA) return i + 2 + ((size_t)v[i + 2] << 8 | v[i + 3]);
  return v.size();
}

// scan + emulation against the serial decoder, every buffer exactly as large as the headers say
void check(const std::vector<uint8_t>& v, int S, long id, bool must_scan) {
  ++g_cases;
  int info[24];
  const long nco = rdp_jpeg_info(v.data(), (long)v.size(), info);
  const long bound = rdp_jpeg_scan_bound(v.data(), (long)v.size());
  if (nco <= 0 || nco > (16L << 20) || bound <= 0) {
    if (must_scan) fail("seed: headers refused", id);
    return;
  }
  std::vector<int> meta(224);
  std::vector<uint8_t> tables((size_t)rdp_jpeg_tables_bytes());
  std::vector<uint8_t> scan((size_t)bound);
  int nbits = -1;
  const int rs = rdp_jpeg_scan(v.data(), (long)v.size(), meta.data(), tables.data(), scan.data(), bound, &nbits);
  if (rs != 0) {
    if (must_scan) fail("seed: scan front end declined", id);
    return;
  }
  ++g_scanned;
  if (nbits < 0 || nbits > bound * 8 || meta[5] * 64L != nco) {
    fail("scan front end: bit count or geometry outside the header's", id);
    return;
  }
  // the tightest buffers the interface allows: the scan's own bytes rounded up to whole words
  const long used = std::max(4L, ((long)nbits / 8 + 3) / 4 * 4);
  std::vector<uint8_t> tight(scan.begin(), scan.begin() + std::min<long>(used, bound));
  tight.resize((size_t)used, 0xA5);
  std::vector<int16_t> got((size_t)nco, (int16_t)0x5A5A), want((size_t)nco);
  int status = -1, stats[2] = {0, 0};
  if (rdp_jpeg_entropy_emulate(tight.data(), used, nbits, tables.data(), meta.data(), got.data(), nco, S, &status,
                               stats) != 0) {
    fail("emulation refused its arguments", id);
    return;
  }
  uint16_t qt[3 * 64];
  const int rd = rdp_jpeg_decode(v.data(), (long)v.size(), want.data(), nco, qt, 0);
  if ((rd != 0) != (status != 0)) {
    fail("verdict differs from rdp_jpeg_decode", id);
    return;
  }
  if (rd != 0) {
    ++g_corrupt;
    return;
  }
  if (std::memcmp(got.data(), want.data(), (size_t)nco * sizeof(int16_t)) != 0) {
    fail("coefficients differ from rdp_jpeg_decode", id);
    return;
  }
  for (int i = 0; i < 3 * 64; ++i)
    if (meta[32 + i] != qt[i]) {
      fail("quantisation tables differ", id);
      return;
    }
  const long n = nbits ? ((long)nbits + (S ? S : 1024) - 1) / (S ? S : 1024) : 1;
  if (stats[0] != n || stats[1] < 0 || stats[1] > 2 * n) fail("statistics outside their bounds", id);
  ++g_equal;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: jpeg_sync_fuzz <seed.jpg> <mutations>\n");
    return 2;
  }
  const std::vector<uint8_t> jpg = read_file(argv[1]);
  const long muts = std::atol(argv[2]);
  if (jpg.empty()) {
    std::printf("cannot read the seed\n");
    return 2;
  }
  const int sizes[4] = {64, 128, 0, 96};
  for (int s = 0; s < 4; ++s) check(jpg, sizes[s], -1 - s, true);
  if (g_equal != 4) fail("seed does not decode equal at every subsequence size", 0);
  const size_t sb = scan_begin(jpg);
  Rng r{0x9E3779B97F4A7C15ull};
  for (long i = 0; i < muts; ++i) check(mutate(jpg, r, (i & 1) ? sb : 0), sizes[(i >> 1) & 3], i, false);
  std::printf("%ld cases, %ld failures (front end took %ld; equal to the serial decode: %ld, corrupt for both: %ld)\n",
              g_cases, g_fail, g_scanned, g_equal, g_corrupt);
  return g_fail ? 1 : 0;
}
