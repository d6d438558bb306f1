// table_images_host.cpp — the staged, receive / transmit and search table
// images checked by their use, on the host (tests/test_table_images.py builds
// this file with lneto_amd/csrc/table_images.cpp by plain g++; no HIP, no
// library).  Each builder must return exactly its layout's total, and every
// region of table_layout.hpp, read through the layout's names the way the
// kernel that owns it combines its lookups (XOR of four byte lookups or of
// eight nibble lookups; the single byte tables by their slicing identities),
// must give Z_k(r) for 4096 registers of a fixed-seed generator plus 0, 1,
// 0x80000000 and 0xFFFFFFFF.  The expected value is gf2.hpp's
// zshift_bytes_fast(r, k), or zshift_bytes(r, k) for the negative k of the F
// and B regions.  A 32-column region must agree in all 32 columns, and the
// regions checked must tile the image: every dword in exactly one.  A region
// that moved (on one side, or in the layout itself: it leaves a gap), a wrong
// total or a region written into another's span fails here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lneto_amd/csrc/gf2.hpp"
#include "../../lneto_amd/csrc/table_images.hpp"
#include "../../lneto_amd/csrc/table_layout.hpp"

using namespace lnx;

namespace {

int g_fail = 0, g_regions = 0;
std::vector<uint32_t> g_regs;

struct Image {
  const char* name;
  std::vector<uint32_t> t;
  uint32_t total;                        // the layout's
  mutable std::vector<uint8_t> cov{};    // how many checked regions hold each dword
  void cover(uint32_t base, uint32_t n) const {
    cov.resize(t.size());
    for (uint32_t i = base; i < base + n && i < cov.size(); ++i) ++cov[i];
  }
  // the builder returned the layout's total, and the regions checked tile it: no gap, no overlap
  void finish() const {
    if (t.size() != total) std::printf("FAIL %s: %zu dwords, layout %u\n", name, t.size(), total), ++g_fail;
    for (size_t i = 0; i < cov.size(); ++i)
      if (cov[i] != 1) {
        std::printf("FAIL %s: dword %zu lies in %d regions\n", name, i, cov[i]), ++g_fail;
        return;
      }
  }
  uint32_t at(uint32_t i) const {
    if (i >= t.size()) {
      std::printf("FAIL %s: dword %u is outside the image (%zu dwords)\n", name, i, t.size());
      std::exit(1);
    }
    return t[i];
  }
};

uint32_t want(uint32_t r, int64_t k) { return k >= 0 ? zshift_bytes_fast(r, (uint64_t)k) : zshift_bytes(r, k); }

// `got(r)` must be Z_k(r) for every register of the set
template <class F>
void check(const Image& im, const char* region, uint32_t idx, int64_t k, F got) {
  ++g_regions;
  for (uint32_t r : g_regs) {
    const uint32_t g = got(r), w = want(r, k);
    if (g != w) {
      std::printf("FAIL %s %s[%u]: Z_%lld(%08x) = %08x, the tables give %08x\n", im.name, region, idx, (long long)k, r, w, g);
      ++g_fail;
      return;
    }
  }
}
// Z_k as four byte tables at base
void byte4(const Image& im, const char* region, uint32_t idx, uint32_t base, int64_t k) {
  im.cover(base, kByte4Dwords);
  check(im, region, idx, k, [&](uint32_t r) {
    uint32_t a = 0;
    for (uint32_t m = 0; m < 4; ++m) a ^= im.at(byte4_at(base, m, (r >> (8 * m)) & 0xFFu));
    return a;
  });
}
// Z_k as eight nibble tables at base
void nib8(const Image& im, const char* region, uint32_t idx, uint32_t base, int64_t k) {
  im.cover(base, kNib8Dwords);
  check(im, region, idx, k, [&](uint32_t r) {
    uint32_t a = 0;
    for (uint32_t i = 0; i < 8; ++i) a ^= im.at(nib8_at(base, i, (r >> (4 * i)) & 15u));
    return a;
  });
}
// ... with every entry in 32 bank columns: each column on its own
void nib8_cols(const Image& im, const char* region, uint32_t base, int64_t k) {
  im.cover(base, kBankCols * kNib8Dwords);
  for (uint32_t c = 0; c < kBankCols; ++c)
    check(im, region, c, k, [&](uint32_t r) {
      uint32_t a = 0;
      for (uint32_t i = 0; i < 8; ++i) a ^= im.at(col_at(base, nib8_at(0, i, (r >> (4 * i)) & 15u), c));
      return a;
    });
}

void stage_image() {
  const Image im{"stage", build_stage_image(), kStageImageDwords};
  // A = Z_2 and B = Z_1 byte tables (stage_research.hip s_z2, s_z1)
  im.cover(kStageAImg, kByteTabDwords), im.cover(kStageBImg, kByteTabDwords);
  check(im, "A/B", 0, 2, [&](uint32_t v) { return (v >> 16) ^ im.at(kStageAImg + (v & 0xFFu)) ^ im.at(kStageBImg + ((v >> 8) & 0xFFu)); });
  check(im, "B", 0, 1, [&](uint32_t v) { return (v >> 8) ^ im.at(kStageBImg + (v & 0xFFu)); });
  // Z_{2^m} by the nibble tables (s_zpow2, s_zd64)
  for (uint32_t m = 0; m < kStageNibLo + kStageNibHi; ++m) {
    im.cover(stage_nib(m, 0, 0), kNib8Dwords);
    check(im, "Z_{2^m}", m, (int64_t)1 << m, [&](uint32_t v) {
      uint32_t a = 0;
      for (uint32_t i = 0; i < 8; ++i) a ^= im.at(stage_nib(m, i, (v >> (4 * i)) & 15u));
      return a;
    });
  }
  byte4(im, "Z4", 0, kStageZ4Img, 4);
  // T8_k[e] = Z_{8-k}(e): the halves of a unit (s_z8half) and Z_1 through T8_7 (s_z1)
  im.cover(kStageZ8Img, 8 * kByteTabDwords);
  for (uint32_t h = 0; h < 2; ++h)
    check(im, "T8 half", h, h ? 4 : 8, [&](uint32_t v) {
      uint32_t a = 0;
      for (uint32_t k = 0; k < 4; ++k) a ^= im.at(kStageZ8Img + kByteTabDwords * (4 * h + k) + ((v >> (8 * k)) & 0xFFu));
      return a;
    });
  check(im, "T8_7", 0, 1, [&](uint32_t v) { return (v >> 8) ^ im.at(kStageZ8Img + kByteTabDwords * 7 + (v & 0xFFu)); });
  for (uint32_t z = 0; z < 3; ++z) byte4(im, "Zx", z, kStageZxImg + kByte4Dwords * z, 16 << z);
  for (uint32_t z = 0; z < 4; ++z) byte4(im, "Zy", z, kStageZyImg + kByte4Dwords * z, 8 * (z + 1));
  im.finish();
}

void rx_image() {
  const Image im{"rx", build_rx_image(), kRxImageDwords};
  byte4(im, "T (Z_128)", 0, kRvImgT, 128);
  byte4(im, "T (Z_124)", 1, kRvImgT + kByte4Dwords, 124);
  for (uint32_t q = 0; q < 32; ++q) nib8(im, "F", q, kRvImgF + kNib8Dwords * q, -8 * (int64_t)q);
  for (uint32_t b = 0; b < 8; ++b) nib8(im, "B", b, kRvImgB + kNib8Dwords * b, -(int64_t)b);
  for (uint32_t m = 0; m < 16; ++m) nib8(im, "P", m, kTxImgP + kNib8Dwords * m, (int64_t)1 << m);
  im.finish();
}

void search_tables() {
  const Image im{"search", build_search_tables(), kSearchTableDwords};
  // the byte step, r -> step[r & 0xFF] ^ (r >> 8): plain, then in every bank column (bstep)
  im.cover(kWordStepOff, kByteTabDwords), im.cover(kSegTabOff, kBankCols * kByteTabDwords);
  check(im, "step", 0, 1, [&](uint32_t r) { return im.at(kWordStepOff + (r & 0xFFu)) ^ (r >> 8); });
  for (uint32_t c = 0; c < kBankCols; ++c)
    check(im, "step columns", c, 1, [&](uint32_t r) { return im.at(col_at(kSegTabOff, r & 0xFFu, c)) ^ (r >> 8); });
  for (uint32_t k = 0; k < 6; ++k) byte4(im, "word levels", k, kWordLevOff + kByte4Dwords * k, 4 << k);
  for (uint32_t k = 0; k < 6; ++k) byte4(im, "24-byte levels", k, kSegLevOff + kByte4Dwords * k, 24 << k);
  byte4(im, "Z_4", 0, kSegZ4Off, 4);
  for (uint32_t k = 0; k < 5; ++k) byte4(im, "48-byte levels", k, kHalfTabOff + kByte4Dwords * k, 48 << k);
  nib8_cols(im, "Z_4 nibble columns", kHalfNibOff, 4);
  byte4(im, "Z_24", 0, kZ24Off, 24);
  nib8_cols(im, "Z_48 nibble columns", kOctNibOff, 48);
  for (uint32_t k = 0; k < 3; ++k) byte4(im, "octet levels", k, kOctLevOff + kByte4Dwords * k, 192 << k);
  im.finish();
}

}  // namespace

int main() {
  g_regs = {0u, 1u, 0x80000000u, 0xFFFFFFFFu};
  uint32_t x = 0x2545F491u;  // xorshift32, fixed seed
  for (int i = 0; i < 4096; ++i) {
    x ^= x << 13, x ^= x >> 17, x ^= x << 5;
    g_regs.push_back(x);
  }
  stage_image();
  rx_image();
  search_tables();
  if (g_fail) return std::printf("%d of %d regions failed\n", g_fail, g_regions), 1;
  std::printf("ok: %d regions, %zu registers each\n", g_regions, g_regs.size());
  return 0;
}
