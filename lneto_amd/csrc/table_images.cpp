// table_images.cpp — the kernels' table images, built once on the host from
// the register algebra of gf2.hpp at the offsets of lds_layout.hpp (the CRC
// rows' LDS images) and table_layout.hpp (the staged, receive / transmit and
// search images).  No HIP here: tests/cpp/table_images_host.cpp and
// tests/cpp/rows_emulator.cpp check the images by their use, without a GPU.
#include "table_images.hpp"
#include <algorithm>
#include "gf2.hpp"
#include "lds_layout.hpp"
#include "table_layout.hpp"

namespace lnx {

namespace {

// x -> Z_k(x) for either sign of k (x^(8k) mod P computed once for k >= 0)
struct Z {
  int64_t k;
  uint32_t p;
  explicit Z(int64_t k_) : k(k_), p(k_ >= 0 ? x8kmodp((uint64_t)k_) : 0u) {}
  uint32_t operator()(uint32_t x) const { return k >= 0 ? multmodp(p, x) : zshift_bytes(x, k); }
};

// The fill forms of table_layout.hpp, each at t: one byte table of Z_k, Z_k as
// four byte tables and as eight nibble tables, and the 32-column forms.
void fill_byte(uint32_t* t, int64_t k) {
  const Z z(k);
  for (uint32_t e = 0; e < 256; ++e) t[e] = z(e);
}
void fill_byte4(uint32_t* t, int64_t k) {
  const Z z(k);
  for (uint32_t m = 0; m < 4; ++m)
    for (uint32_t e = 0; e < 256; ++e) t[byte4_at(0, m, e)] = z(e << (8 * m));
}
void fill_nib8(uint32_t* t, int64_t k) {
  const Z z(k);
  for (uint32_t i = 0; i < 8; ++i)
    for (uint32_t v = 0; v < 16; ++v) t[nib8_at(0, i, v)] = z(v << (4 * i));
}
// n entries at src, each into its 32 bank columns at t
void fill_cols(uint32_t* t, const uint32_t* src, uint32_t n) {
  for (uint32_t x = 0; x < n; ++x) std::fill_n(t + col_at(0, x, 0), kBankCols, src[x]);
}
void fill_byte_cols(uint32_t* t, int64_t k) {
  uint32_t one[kByteTabDwords];
  fill_byte(one, k);
  fill_cols(t, one, kByteTabDwords);
}
void fill_nib8_cols(uint32_t* t, int64_t k) {
  uint32_t one[kNib8Dwords];
  fill_nib8(one, k);
  fill_cols(t, one, kNib8Dwords);
}
// the U region of an LDS image (lds_layout.hpp): Z_k as four byte tables in 32 lane-private columns
void fill_u(std::vector<uint32_t>& img, int64_t k) {
  uint32_t one[kByte4Dwords];
  fill_byte4(one, k);
  for (uint32_t m = 0; m < 4; ++m)
    for (uint32_t e = 0; e < 256; ++e)
      for (uint32_t c = 0; c < 32; ++c) img[u_addr(m, e, c) / 4] = one[byte4_at(0, m, e)];
}

}  // namespace

// The 160 KiB LDS image of row width rl (lds_layout.hpp): U = Z_SB, F_p = Z_{-4p}, T = Z_{-t}.
std::vector<uint32_t> build_lds_image(uint32_t rl) {
  std::vector<uint32_t> img(kLdsDwords, 0);
  fill_u(img, 4 * (int64_t)rl);
  for (uint32_t c = 0; c < 32; ++c) {
    const int64_t p = c % rl;
    for (uint32_t i = 0; i < 8; ++i)
      for (uint32_t v = 0; v < 16; ++v) img[f_addr(c, i, v) / 4] = zshift_bytes(v << (4 * i), -4 * p);
    const uint32_t q0 = (uint32_t)p & 7u;
    for (uint32_t h = 0; h < 2; ++h)
      for (uint32_t t = 1; t < 4; ++t)
        for (uint32_t v = 0; v < 16; ++v)
          img[t_addr(c, h, t, v) / 4] = zshift_bytes(v << (4 * (q0 + 4 * h)), -(int64_t)t);
  }
  return img;
}

#ifdef LNX_RESEARCH
// The LDS image of the streaming rows (stream_rows.hpp) with row steps of sb
// bytes (128: 8-lane rows, 64: 4-lane rows): U = Z_4 (the chain's dword step),
// F column n = Z_{-4n} (n = 0..31), then the Z_{sb-12} byte tables (the skip
// over the other lanes' pieces, at kSZ116), Z_c (c = 0..3) and Z_{sb-4k}
// (k = 0..4) nibble tables by row lane, the constants Z_{sb-j}(0xFFFFFFFF) and
// the Z_1 byte table.
std::vector<uint32_t> build_stream_image(int64_t sb) {
  std::vector<uint32_t> img(kLdsDwords, 0);
  uint32_t* t = img.data();
  fill_u(img, 4);
  for (uint32_t c = 0; c < 32; ++c)
    for (uint32_t i = 0; i < 8; ++i)
      for (uint32_t v = 0; v < 16; ++v) img[f_addr(c, i, v) / 4] = zshift_bytes(v << (4 * i), -4 * (int64_t)c);
  fill_byte4(t + kSZ116 / 4, sb - 12);
  for (uint32_t c = 0; c < 4; ++c) fill_nib8(t + kSTc / 4 + kNib8Dwords * c, c);
  for (uint32_t k = 0; k < 5; ++k) fill_nib8(t + kSG / 4 + kNib8Dwords * k, sb - 4 * (int64_t)k);
  for (uint32_t j = 0; j < 16; ++j) img[kSK / 4 + j] = zshift_bytes(0xFFFFFFFFu, sb - (int64_t)j);
  fill_byte(t + kST1 / 4, 1);
  return img;
}

// The LDS image of the lane streams (stream_lanes.hpp): U = Z_4, then the
// Z_c byte tables (c = 1..3), the Z_{64-4k} nibble tables (k = 0..15) and
// the constants Z_{64-j}(0xFFFFFFFF) (lds_layout.hpp kLZc, kLZd, kLK).
std::vector<uint32_t> build_lanes_image() {
  std::vector<uint32_t> img(kLdsDwords, 0);
  uint32_t* t = img.data();
  fill_u(img, 4);
  for (uint32_t c = 1; c < 4; ++c) fill_byte4(t + kLZc / 4 + kByte4Dwords * (c - 1), c);
  for (uint32_t k = 0; k < 16; ++k) fill_nib8(t + kLZd / 4 + kNib8Dwords * k, 64 - 4 * (int64_t)k);
  for (uint32_t j = 0; j < 64; ++j) img[kLK / 4 + j] = zshift_bytes(0xFFFFFFFFu, 64 - (int64_t)j);
  return img;
}
#endif  // LNX_RESEARCH

// Compact form of an image (lds_layout.hpp kCompactDwords): the U values once,
// then the F/T tail verbatim.
static std::vector<uint32_t> compact_image(const std::vector<uint32_t>& full) {
  std::vector<uint32_t> c(kCompactDwords);
  for (uint32_t m = 0; m < 4; ++m)
    for (uint32_t e = 0; e < 256; ++e) c[256 * m + e] = full[u_addr(m, e, 0) / 4];
  std::copy(full.begin() + kFBase / 4, full.end(), c.begin() + kCompactUDwords);
  return c;
}

// The compact images back to back: [RL = 16][RL = 4][RL = 32][stream][stream64][lanes] (lds_layout.hpp image_index).
const std::vector<uint32_t>& host_image() {
  static const std::vector<uint32_t> img = [] {
    std::vector<uint32_t> all;
    auto add = [&all](const std::vector<uint32_t>& full) {
      const std::vector<uint32_t> im = compact_image(full);
      all.insert(all.end(), im.begin(), im.end());
    };
    for (uint32_t rl : {16u, 4u, 32u}) add(build_lds_image(rl));  // the product's row widths (image_index 0..2)
#ifdef LNX_RESEARCH
    add(build_stream_image(128));  // image_index 3, 4: the stream images (128- and 64-byte row steps)
    add(build_stream_image(64));
    add(build_lanes_image());      // 5
#endif
    return all;
  }();
  return img;
}

// The staged lane streams' image (table_layout.hpp kStage*).
std::vector<uint32_t> build_stage_image() {
  std::vector<uint32_t> img(kStageImageDwords);
  uint32_t* t = img.data();
  fill_byte(t + kStageAImg, 2);
  fill_byte(t + kStageBImg, 1);
  for (uint32_t m = 0; m < kStageNibLo + kStageNibHi; ++m) fill_nib8(t + stage_nib(m, 0, 0), (int64_t)1 << m);
  fill_byte4(t + kStageZ4Img, 4);
  for (uint32_t k = 0; k < 8; ++k) fill_byte(t + kStageZ8Img + kByteTabDwords * k, 8 - (int64_t)k);
  for (uint32_t z = 0; z < 3; ++z) fill_byte4(t + kStageZxImg + kByte4Dwords * z, 16 << z);
  for (uint32_t z = 0; z < 4; ++z) fill_byte4(t + kStageZyImg + kByte4Dwords * z, 8 * (z + 1));
  return img;
}

// The receive / transmit image (table_layout.hpp kRvImg*, kTxImgP).
std::vector<uint32_t> build_rx_image() {
  std::vector<uint32_t> img(kRxImageDwords);
  uint32_t* t = img.data();
  fill_byte4(t + kRvImgT, 128);
  fill_byte4(t + kRvImgT + kByte4Dwords, 124);
  for (uint32_t q = 0; q < 32; ++q) fill_nib8(t + kRvImgF + kNib8Dwords * q, -8 * (int64_t)q);
  for (uint32_t b = 0; b < 8; ++b) fill_nib8(t + kRvImgB + kNib8Dwords * b, -(int64_t)b);
  for (uint32_t m = 0; m < 16; ++m) fill_nib8(t + kTxImgP + kNib8Dwords * m, (int64_t)1 << m);
  return img;
}

// The RST reply image (table_layout.hpp kRstImgZ).
std::vector<uint32_t> build_rst_image() {
  std::vector<uint32_t> img(kRstImageDwords);
  for (uint32_t p = 0; p < kRstLanes; ++p) {
    const Z z(4 * (int64_t)(kRstLanes - p));
    for (uint32_t i = 0; i < 8; ++i)
      for (uint32_t v = 0; v < 16; ++v) img[rst_nib(p, i, v)] = z(v << (4 * i));
  }
  return img;
}

// The echo reply image (table_layout.hpp kEchoImgZ).
std::vector<uint32_t> build_echo_image() {
  std::vector<uint32_t> img(kEchoImageDwords);
  for (uint32_t t = 1; t <= kEchoZ; ++t) {
    const Z z(4 * (int64_t)t);
    for (uint32_t i = 0; i < 8; ++i)
      for (uint32_t v = 0; v < 16; ++v) img[echo_nib(t, i, v)] = z(v << (4 * i));
  }
  fill_byte4(img.data() + kEchoImgB, 4 * (int64_t)kEchoZ);
  return img;
}

// The CRC32Search tables (table_layout.hpp k*Off).
std::vector<uint32_t> build_search_tables() {
  std::vector<uint32_t> img(kSearchTableDwords);
  uint32_t* t = img.data();
  fill_byte(t + kWordStepOff, 1);
  for (uint32_t k = 0; k < 6; ++k) fill_byte4(t + kWordLevOff + kByte4Dwords * k, 4 << k);
  fill_byte_cols(t + kSegTabOff, 1);
  for (uint32_t k = 0; k < 6; ++k) fill_byte4(t + kSegLevOff + kByte4Dwords * k, 24 << k);
  fill_byte4(t + kSegZ4Off, 4);
  for (uint32_t k = 0; k < 5; ++k) fill_byte4(t + kHalfTabOff + kByte4Dwords * k, 48 << k);
  fill_nib8_cols(t + kHalfNibOff, 4);
  fill_byte4(t + kZ24Off, 24);
  fill_nib8_cols(t + kOctNibOff, 48);
  for (uint32_t k = 0; k < 3; ++k) fill_byte4(t + kOctLevOff + kByte4Dwords * k, 192 << k);
  return img;
}

}  // namespace lnx
