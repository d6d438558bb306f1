// table_layout.hpp — dword layout of the table images that table_images.cpp
// builds on the host and the kernels read from HBM: the staged lane streams'
// image, the receive / transmit image, the CRC32Search tables and the RST and
// echo reply images.  (The CRC
// rows' LDS images are in lds_layout.hpp.)  Each region starts where the one
// before it ends; both sides take every offset from here.
//
// Every region is Z_k (gf2.hpp) in one of two decompositions:
//   byte tables    Z_k(x) = XOR_m B_m[byte m of x],   B_m[e] = Z_k(e << 8m), entry (m, e) at 256 m + e
//   nibble tables  Z_k(x) = XOR_i N_i[nibble i of x], N_i[v] = Z_k(v << 4i), entry (i, v) at 16 i + v
// and some are replicated over the 32 LDS bank columns, entry x of column c at
// 32 x + c, so a kernel copies them to LDS verbatim and lane l reads column
// l % 32 without bank conflicts.
#pragma once
#include <cstdint>

namespace lnx {

constexpr uint32_t kByteTabDwords = 256;                  // one byte table
constexpr uint32_t kByte4Dwords = 4 * kByteTabDwords;     // Z_k as four byte tables
constexpr uint32_t kNib8Dwords = 8 * 16;                  // Z_k as eight nibble tables
constexpr uint32_t kBankCols = 32;
constexpr uint32_t byte4_at(uint32_t base, uint32_t m, uint32_t e) { return base + kByteTabDwords * m + e; }
constexpr uint32_t nib8_at(uint32_t base, uint32_t i, uint32_t v) { return base + 16u * i + v; }
constexpr uint32_t col_at(uint32_t base, uint32_t x, uint32_t c) { return base + kBankCols * x + c; }

// ---- the staged lane streams' image (stage_kernel.hip, research/stage_research.hip)
constexpr uint32_t kStageAImg = 0;                                      // A[e] = Z_2(e): the research FOLD 2 / 4 kernels
constexpr uint32_t kStageBImg = kStageAImg + kByteTabDwords;            // B[e] = Z_1(e): the same
constexpr uint32_t kStageNibLo = 31;                                    // Z_{2^m}, m < 31, go to LDS; m = 31..39 stay in HBM
constexpr uint32_t kStageNibImg = kStageBImg + kByteTabDwords;          // Z_{2^m} nibble tables, m = 0..30: the carries' Z_d
constexpr uint32_t kStageZ4Img = kStageNibImg + kStageNibLo * kNib8Dwords;  // Z_4 byte tables: research FOLD 4
constexpr uint32_t kStageZ8Img = kStageZ4Img + kByte4Dwords;            // T8_k[e] = Z_{8-k}(e), k < 8, at 256 k + e: the product fold
constexpr uint32_t kStageZxImg = kStageZ8Img + 8 * kByteTabDwords;      // Z_16, Z_32, Z_64 byte tables: research DEFER
constexpr uint32_t kStageZyImg = kStageZxImg + 3 * kByte4Dwords;        // Z_8, Z_16, Z_24, Z_32 byte tables: research two chains
constexpr uint32_t kStageNibHiImg = kStageZyImg + 4 * kByte4Dwords;     // Z_{2^m} nibble tables, m = 31..39: giant frames' Z_d
constexpr uint32_t kStageNibHi = 9;
constexpr uint32_t kStageImageDwords = kStageNibHiImg + kStageNibHi * kNib8Dwords;
// nibble table i, entry v of Z_{2^m}, m < 40
constexpr uint32_t stage_nib(uint32_t m, uint32_t i, uint32_t v) {
  return nib8_at(m < kStageNibLo ? kStageNibImg + kNib8Dwords * m : kStageNibHiImg + kNib8Dwords * (m - kStageNibLo), i, v);
}

// ---- the receive / transmit image (rx_verify_kernel.hip: rx_verify_kernel, tx_finish_kernel)
constexpr uint32_t kRvImgT = 0;                                 // T_k = Z_128, T_{4+k} = Z_124 byte tables (k < 4): the rows' fold
constexpr uint32_t kRvImgF = kRvImgT + 2 * kByte4Dwords;        // F_q = Z_{-8q} nibble tables, q < 32: a lane's final alignment
constexpr uint32_t kRvImgB = kRvImgF + 32 * kNib8Dwords;        // B_b = Z_{-b} nibble tables, b < 8: the frame end inside a qword
constexpr uint32_t kTxImgP = kRvImgB + 8 * kNib8Dwords;         // Z_{2^m} nibble tables, m < 16: tx_finish's CRC corrections
constexpr uint32_t kRxImageDwords = kTxImgP + 16 * kNib8Dwords;

// ---- the CRC32Search tables (search_kernel.hip, research/search_research.inc)
constexpr uint32_t kWordStepOff = 0;                                    // Z_1 byte table (the byte step): research word lanes
constexpr uint32_t kWordLevOff = kWordStepOff + kByteTabDwords;         // Z_{4*2^k} byte tables, k < 6: the same
constexpr uint32_t kWordTabDwords = kWordLevOff + 6 * kByte4Dwords - kWordStepOff;
constexpr uint32_t kSegTabOff = kWordStepOff + kWordTabDwords;          // the byte step in 32 columns: research 24- / 48-byte lanes
constexpr uint32_t kSegLevOff = kSegTabOff + kBankCols * kByteTabDwords;  // Z_{24*2^k} byte tables, k < 6: research 24-byte lanes
constexpr uint32_t kSegZ4Off = kSegLevOff + 6 * kByte4Dwords;           // Z_4 byte tables: every kernel's U values (the product's too)
constexpr uint32_t kSegTabDwords = kSegZ4Off + kByte4Dwords - kSegTabOff;  // (the 24-byte lanes copy the three in one piece)
constexpr uint32_t kHalfTabOff = kSegTabOff + kSegTabDwords;            // Z_{48*2^k} byte tables, k < 5: research 48-byte lanes
constexpr uint32_t kHalfNibOff = kHalfTabOff + 5 * kByte4Dwords;        // Z_4 nibble tables in 32 columns: the same (pass B)
constexpr uint32_t kZ24Off = kHalfNibOff + kBankCols * kNib8Dwords;     // Z_24 byte tables: research split chains
constexpr uint32_t kOctNibOff = kZ24Off + kByte4Dwords;                 // Z_48 nibble tables in 32 columns: the product (octets)
constexpr uint32_t kOctLevOff = kOctNibOff + kBankCols * kNib8Dwords;   // Z_{192*2^k} byte tables, k < 3: the product's scan
constexpr uint32_t kOctTabDwords = kOctLevOff + 3 * kByte4Dwords - kOctNibOff;  // (copied in one piece)
constexpr uint32_t kSearchTableDwords = kOctNibOff + kOctTabDwords;

// ---- the RST reply image, of any 60-byte frame in a 64-byte slot (slot_frame.hpp slot_fcs_part: RST and ARP replies)
constexpr uint32_t kRstLanes = 15;                                      // the dwords of a 60-byte frame
constexpr uint32_t kRstImgZ = 0;                                        // Z_{4(15-p)} nibble tables, p < 15: dword p's share of the FCS
constexpr uint32_t kRstImageDwords = kRstImgZ + kRstLanes * kNib8Dwords;
// (an odd p keeps its nibble tables in swapped pairs: the sixteen lanes of a row, one p each, reach all 32 LDS banks)
constexpr uint32_t rst_nib(uint32_t p, uint32_t i, uint32_t v) { return nib8_at(kRstImgZ + kNib8Dwords * p, i ^ (p & 1u), v); }
static_assert(kRstImageDwords == 1920, "RST reply image");

// ---- the echo reply image (echo_kernel.hip: echo_plan.hpp echo_fcs_part)
constexpr uint32_t kEchoZ = 64;                                         // the dwords a wave folds in one step
constexpr uint32_t kEchoImgZ = 0;                                       // Z_{4t} nibble tables, 1 <= t <= 64: the share of a dword t dwords before the end
constexpr uint32_t kEchoImgB = kEchoImgZ + kEchoZ * kNib8Dwords;         // Z_256 byte tables: a lane's own register over one more step of the wave
constexpr uint32_t kEchoImageDwords = kEchoImgB + kByte4Dwords;
// (an odd t keeps its nibble tables in swapped pairs, as the RST image does)
constexpr uint32_t echo_nib(uint32_t t, uint32_t i, uint32_t v) { return nib8_at(kEchoImgZ + kNib8Dwords * (t - 1u), i ^ (t & 1u), v); }
static_assert(kEchoImgB == 8192 && kEchoImageDwords == 9216, "echo reply image");

// the values every reader of these images was written against
static_assert(kStageZ8Img == 5504 && kStageNibHiImg == 14720 && kStageImageDwords == 15872, "staged image");
static_assert(kRvImgF == 2048 && kTxImgP == 7168 && kRxImageDwords == 9216, "receive / transmit image");
static_assert(kSegTabOff == 6400 && kHalfTabOff == 21760 && kOctNibOff == 32000 && kSearchTableDwords == 39168,
              "search tables");

}  // namespace lnx
