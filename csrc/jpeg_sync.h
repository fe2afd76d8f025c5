// Self-synchronising parallel Huffman decode of one marker-less baseline JPEG scan (after Weissenberger &
// Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018, and their GPU JPEG decoder): the
// per-lane core, host + device. The HIP kernels (jpeg_entropy.hip), the CPU emulation and the sanitizer
// build (jpeg.cpp, tests/native/jpeg_sync_fuzz_main.cpp) all run these functions.
//
// The scan is cut into subsequences of S bits; one lane owns one subsequence. A lane's decoder state is
// (bit position p, block index within the MCU b, zig-zag index k). Lane t first decodes from the guess
// (t * S, 0, 0), then repeatedly from lane t - 1's end state until nothing changes: lane 0 is right from
// the start, so after i rounds the first i + 1 subsequences are (jpeg_entropy.hip has the loop bounds).
//
// The scan buffer holds the entropy-coded bytes with the 0xFF00 stuffing removed, cut at the first
// marker (rdp_jpeg_scan). It is read through aligned 32-bit words below ceil(nbits / 32) (struct Bits);
// every bit at or past `nbits` reads as zero -- what the host decoder feeds once it runs into a marker or the end.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RDP_HD __host__ __device__ inline
#else
#define RDP_HD inline
#endif

namespace jsync {

constexpr int kLanes = 1024;     // subsequences per workgroup (one lane each)
constexpr int kDefaultBits = 1024;  // S when the caller passes 0 (profiles/jpeg_gpu_entropy.md)

// One Huffman table as jpeg.cpp's Huff decodes it: 9-bit lookahead ((length << 8) | value, 0: not in the
// table), then the canonical search over code lengths 10..16.
struct HuffTab {
  uint16_t look[512];
  int32_t maxcode[17], mincode[17], valptr[17];
  uint8_t vals[256];
};

// The table block (one H2D copy; the kernels stage it in LDS): tables 0-1 DC, 2-3 AC; per block of an MCU
// its tables (dc | ac << 4), component and position inside the MCU; the zig-zag order.
struct Tables {
  HuffTab t[4];
  uint8_t sel[12], comp[12], by[12], bx[12];
  uint8_t zz[64];
  int32_t nb;  // blocks per MCU
  int32_t pad[3];
};
static_assert(sizeof(Tables) % 16 == 0, "staged as 16-byte words");

struct St {
  uint32_t p;   // bit position
  uint32_t bk;  // (b << 6) | k
};
RDP_HD bool same(St a, St b) { return a.p == b.p && a.bk == b.bk; }

// what the write pass needs of the geometry block (rdp_jpeg_meta's int32[32])
struct Geo {
  int nb, mcux;
  long total, cap;  // blocks in the frame / in the output buffer
  int h[3], v[3], bw[3], first[3];
};
RDP_HD Geo make_geo(const int* g, int nb, long cap_blocks) {
  Geo o;
  o.nb = nb;
  o.total = g[5];
  o.cap = cap_blocks;
  for (int c = 0; c < 3; ++c) {
    o.h[c] = g[8 + 8 * c];
    o.v[c] = g[9 + 8 * c];
    o.bw[c] = g[10 + 8 * c];
    o.first[c] = g[12 + 8 * c];
  }
  o.mcux = o.h[0] > 0 ? o.bw[0] / o.h[0] : 1;
  if (o.mcux < 1) o.mcux = 1;
  return o;
}

// Bit reader over the scan words (MSB first): 64 bits in registers, refilled one aligned word at a time,
// the next word loaded one refill ahead so that its latency hides behind the symbols in between. Words at
// or past ceil(nbits / 32) are never loaded; every bit at or past nbits reads as zero.
struct Bits {
  const uint32_t* w;
  uint32_t nbits, nw;
  uint32_t p;    // position of the first bit of acc
  uint64_t acc;  // the next `have` bits, MSB-aligned
  int have;      // >= 32 between calls
  uint32_t wi, nxt;  // the next word to take in, already loaded

  RDP_HD uint32_t word(uint32_t i) const {
    if (i >= nw) return 0u;
    uint32_t v = __builtin_bswap32(w[i]);
    const uint32_t end = (i + 1) * 32;
    if (end > nbits) v &= ~0u << (end - nbits);  // 1..31: word i holds at least one of the frame's bits
    return v;
  }
  RDP_HD Bits(const uint32_t* words, uint32_t bits, uint32_t pos) : w(words), nbits(bits), nw((bits + 31) >> 5), p(pos) {
    const uint32_t i = pos >> 5;
    acc = (((uint64_t)word(i) << 32) | word(i + 1)) << (pos & 31);
    have = 64 - (int)(pos & 31);
    wi = i + 2;
    nxt = word(wi);
  }
  RDP_HD uint32_t peek32() const { return (uint32_t)(acc >> 32); }
  RDP_HD void skip(int n) {  // n <= 31
    acc <<= n;
    have -= n;
    p += (uint32_t)n;
    if (have < 32) {  // 1 <= have here: at least 32 before, at most 31 taken
      acc |= (uint64_t)nxt << (32 - have);
      have += 32;
      ++wi;
      nxt = word(wi);
    }
  }
};

enum { kDone = 1, kErr = 2, kVal = 4 };

// One symbol (Huffman code + magnitude bits) at s. kVal: coefficient `val` at zig-zag index `zk` (the DC
// difference at 0); kDone: the block ended; kErr: decode_segment's error conditions -- an invalid code
// (consumes one bit), a DC size above 11, k overrunning 63 (both consume the symbol; the latter ends
// the block). Every call advances p by at least 1.
RDP_HD int step(const Tables& T, Bits& br, uint32_t& bk, int& zk, int& val) {
  const uint32_t v = br.peek32();
  int b = (int)(bk >> 6), k = (int)(bk & 63);
  const int sel = T.sel[b];
  const HuffTab& h = T.t[k == 0 ? (sel & 1) : 2 + ((sel >> 4) & 1)];
  int l = 0, sym = 0;
  const uint32_t e = h.look[v >> 23];
  if (e) {
    l = (int)(e >> 8);
    sym = (int)(e & 255);
  } else {
    for (int i = 10; i <= 16; ++i) {
      const int c = (int)(v >> (32 - i));
      if (h.maxcode[i] >= 0 && c <= h.maxcode[i] && c >= h.mincode[i]) {
        l = i;
        sym = h.vals[(h.valptr[i] + c - h.mincode[i]) & 255];
        break;
      }
    }
    if (!l) {
      br.skip(1);
      return kErr;
    }
  }
  const int sz = sym & 15;
  const uint32_t mag = sz ? (v << l) >> (32 - sz) : 0u;
  const int ext = (sz && mag < (1u << (sz - 1))) ? (int)mag - (1 << sz) + 1 : (int)mag;
  int f = 0;
  if (k == 0) {
    if (sym > 11) {
      f = kErr;
    } else {
      f = kVal;
      zk = 0;
      val = ext;
    }
    br.skip(l + sz);
    k = 1;
  } else if (sz == 0) {
    br.skip(l);
    k = (sym >> 4) == 15 ? k + 16 : 64;  // ZRL / EOB
  } else {
    br.skip(l + sz);
    k += sym >> 4;
    if (k > 63) {
      f = kErr;
      k = 64;
    } else {
      f = kVal;
      zk = k;
      val = ext;
      ++k;
    }
  }
  if (k >= 64) {
    f |= kDone;
    k = 0;
    b = b + 1 >= T.nb ? 0 : b + 1;
  }
  bk = ((uint32_t)b << 6) | (uint32_t)k;
  return f;
}

// first bit after subsequence t of n
RDP_HD uint32_t sub_end(uint32_t t, uint32_t n, uint32_t S, uint32_t nbits) { return t + 1 >= n ? nbits : (t + 1) * S; }
RDP_HD uint32_t sub_count(uint32_t nbits, uint32_t S) { return nbits ? (nbits + S - 1) / S : 1u; }

// Speculative run: every symbol that starts before end_bit; errors raise nothing. Returns the blocks
// completed. At most end_bit - s.p steps.
RDP_HD int run_spec(const Tables& T, const uint32_t* w, uint32_t nbits, St& s, uint32_t end_bit) {
  int blocks = 0, zk = 0, val = 0;
  Bits br(w, nbits, s.p);
  while (br.p < end_bit) blocks += step(T, br, s.bk, zk, val) & kDone;
  s.p = br.p;
  return blocks;
}

// block ordinal (scan order) -> block index in the coefficient planes, as decode_segment walks them
RDP_HD long block_index(const Tables& T, const Geo& g, long ord) {
  const long m = ord / g.nb;
  const int b = (int)(ord - m * g.nb);
  const int c = T.comp[b];
  const long my = m / g.mcux, mx = m - my * g.mcux;
  return g.first[c] + (my * g.v[c] + T.by[b]) * g.bw[c] + mx * g.h[c] + T.bx[b];
}

// Write run from a synchronised start: `ord` is the ordinal of the block in progress at s. Stores every
// AC value and the DC difference of blocks below g.total; stops at g.total, at end_bit (unless `last`:
// the last subsequence runs on over zero bits, the host's truncated-scan behaviour) or at an error
// (returns 1). At most 64 symbols per remaining block.
RDP_HD int run_write(const Tables& T, const Geo& g, const uint32_t* w, uint32_t nbits, St s, uint32_t end_bit,
                     bool last, long ord, int16_t* out) {
  if (ord >= g.total) return 0;
  long budget = (g.total - ord) * 64;
  long blk = block_index(T, g, ord);
  int zk = 0, val = 0;
  Bits br(w, nbits, s.p);
  while (ord < g.total && (last || br.p < end_bit) && budget-- > 0) {
    const int f = step(T, br, s.bk, zk, val);
    if (f & kErr) return 1;
    if ((f & kVal) && blk >= 0 && blk < g.cap) out[blk * 64 + T.zz[zk]] = (int16_t)val;
    if (f & kDone) {
      ++ord;
      if (ord < g.total) blk = block_index(T, g, ord);
    }
  }
  return 0;
}

// DC prediction: the j-th block of component c in scan order -> block index
RDP_HD long dc_block_index(const Geo& g, int c, long j) {
  const int hv = g.h[c] * g.v[c];
  const long m = j / hv;
  const int i = (int)(j - m * hv);
  const long my = m / g.mcux, mx = m - my * g.mcux;
  return g.first[c] + (my * g.v[c] + i / g.h[c]) * g.bw[c] + mx * g.h[c] + i % g.h[c];
}

// work buffer (int32 words) for a scan capacity of cap_bytes at S bits per subsequence: per subsequence
// the start state, the end state, the blocks completed and the first block ordinal; per workgroup the
// rounds it took; then (subsequences, rounds).
struct Work {
  long nsub, nwg;
  long in, end, cnt, ord, wgr, stats, words;
};
RDP_HD Work work_layout(long cap_bytes, int S) {
  Work k;
  k.nsub = (cap_bytes * 8 + S - 1) / S;
  if (k.nsub < 1) k.nsub = 1;
  k.nwg = (k.nsub + kLanes - 1) / kLanes;
  k.in = 0;
  k.end = k.in + 2 * k.nsub;
  k.cnt = k.end + 2 * k.nsub;
  k.ord = k.cnt + k.nsub;
  k.wgr = k.ord + k.nsub;
  k.stats = k.wgr + k.nwg;
  k.words = k.stats + 4;
  return k;
}

}  // namespace jsync
