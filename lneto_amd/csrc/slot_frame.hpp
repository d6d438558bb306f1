// slot_frame.hpp — a frame of 60 bytes in a 64-byte slot:
// fifteen little-endian dwords that a protocol's plan header gives one at a
// time (reply_plan.hpp rst_word, arp_plan.hpp arp_word), and a sixteenth that
// holds the FCS, or zero without one.  What belongs to the slot and not to the
// protocol stands here once: the slot's constants, a dword's share of the FCS
// over the kRstImgZ tables (table_layout.hpp), the host's per-frame form
// (reply_host.cpp, arp_host.cpp) and, for the kernels, the geometry, the table
// copy, the 16-lane row stage, the explicit-entries kernel body and the launch
// of a kernel's FCS form or its plain form.  The first part is plain C++17
// that a host compiler also accepts (tests/cpp/reply_plan_host.cpp,
// tests/cpp/arp_plan_host.cpp).
#pragma once
#include <cstdint>
#include <vector>
#include "table_images.hpp"
#include "table_layout.hpp"
#include "wave_util.hpp"

namespace lnx {

constexpr uint32_t kSlotWords = 16, kSlotPadded = 60;
static_assert(kSlotWords == kRstLanes + 1u && kSlotPadded == 4u * kRstLanes, "the FCS tables are the 60-byte frame's");

// two big-endian 16-bit fields as the little-endian dword that holds them in memory
LNX_HD uint32_t slot_pack(uint32_t f0, uint32_t f1) {
  return ((f0 >> 8) & 0xFFu) | ((f0 & 0xFFu) << 8) | (((f1 >> 8) & 0xFFu) << 16) | ((f1 & 0xFFu) << 24);
}

// The FCS of the 60 bytes.  Processing a dword w at register r is Z_4(r ^ w)
// (gf2.hpp), so the register after the fifteen dwords is
//   XOR_p Z_{4 (15 - p)}(w_p)  ^  Z_60(0xFFFFFFFF),
// the init folded into dword 0, and the CRC its complement.  tab(p, i, v): entry
// v of nibble table i of Z_{4 (15 - p)} (table_layout.hpp kRstImgZ).
template <class Tab>
LNX_HD uint32_t slot_fcs_part(uint32_t p, uint32_t word, Tab tab) {
  const uint32_t w = p == 0 ? ~word : word;
  uint32_t z = 0;
  for (uint32_t i = 0; i < 8; ++i) z ^= tab(p, i, (w >> (4 * i)) & 15u);
  return z;
}

// One slot on the host: out[0 .. 63] from word(p), the frame's dword p < 15; the
// frame's length, 64 with the FCS and 60 without (the slot's last dword is then 0).
template <class Word>
inline uint32_t slot_frame(bool fcs, uint8_t out[64], Word word) {
  static const std::vector<uint32_t> image = build_rst_image();
  auto tab = [&](uint32_t p, uint32_t i, uint32_t v) -> uint32_t { return image[rst_nib(p, i, v)]; };
  uint32_t reg = 0;
  for (uint32_t p = 0; p < kSlotWords; ++p) {
    uint32_t w = 0;
    if (p < kRstLanes) {
      w = word(p);
      reg ^= slot_fcs_part(p, w, tab);
    } else if (fcs) {
      w = ~reg;
    }
    for (uint32_t b = 0; b < 4; ++b) out[4 * p + b] = (uint8_t)(w >> (8 * b));  // little-endian dwords
  }
  return fcs ? 64u : kSlotPadded;
}

#if defined(__HIPCC__)
// (restated in tests/test_rst_reply_gpu.py, tests/test_rst_reply_grid_mid.py and tests/test_arp_reply_gpu.py)
constexpr int kSlotBlock = 256;                // frames per chunk: one per thread (tests: CHUNK)
constexpr uint32_t kSlotWaves = kSlotBlock / 64, kSlotRows = kSlotBlock / 16;
constexpr uint32_t kSlotGridCap = 512;         // workgroups of the count / build launches (tests: GRID_CAP)
constexpr uint32_t kSlotFramesGridCap = 2048;  // ... of the explicit-entries launch, grid-strided past it (tests: FRAMES_GRID_CAP)
static_assert(kSlotBlock == 64 * (int)kSlotWaves && kSlotBlock == 16 * (int)kSlotRows,
              "whole waves, and a 16-lane row a thread group: slot_rows and slot_tables stride by these");

// the FCS tables into LDS: every thread of the kSlotBlock, before the barrier ahead of the first slot_rows
__device__ __forceinline__ void slot_tables(uint32_t* tab, const uint32_t* __restrict__ image) {
  for (uint32_t i = threadIdx.x; i < kRstImageDwords; i += kSlotBlock) tab[i] = image[kRstImgZ + i];
}

// the dword of this thread's lane in its row: lanes 0 .. 14 their own, lane 15 (the FCS) goes through dword 14's motions
__device__ __forceinline__ uint32_t slot_lane_word() {
  const uint32_t p = threadIdx.x & 15u;
  return p < kRstLanes ? p : kRstLanes - 1u;
}

// The row stage.  Replies k0 .. k0 + m - 1 from the staged entries 0 .. m - 1:
// row `row` takes entries row, row + 16, ...; lane p of the row makes dword p,
// word(pw, j, live) with pw = slot_lane_word() (the caller hoists what of the
// dword the entry does not decide), the row XORs the fifteen shares of the FCS
// and lane 15 holds its complement.  The row's sixteen stores are one whole
// aligned 64-byte block; a row past m stores nothing.  An entry that clears
// `live` becomes sixteen zero dwords.  m <= kSlotBlock.
template <bool FCS, class Word>
__device__ __forceinline__ void slot_rows(const uint32_t* tab, uint32_t m, uint64_t k0, uint32_t* __restrict__ reply, Word word) {
  const uint32_t p = threadIdx.x & 15u, row = threadIdx.x >> 4;
  const uint32_t pw = slot_lane_word();
  for (uint32_t j0 = 0; j0 < m; j0 += kSlotRows) {  // (uniform: m <= kSlotBlock, so j < kSlotBlock)
    const uint32_t j = j0 + row;
    bool live = true;
    uint32_t w = word(pw, j, live);
    if (FCS) {
      uint32_t z = slot_fcs_part(pw, w, [tab](uint32_t q, uint32_t i, uint32_t v) -> uint32_t { return tab[rst_nib(q, i, v)]; });
      z = row_xor16(p < kRstLanes ? z : 0u);
      w = p < kRstLanes ? w : ~z;
    } else {
      w = p < kRstLanes ? w : 0u;
    }
    if (j < m) reply[(k0 + j) * kSlotWords + p] = live ? w : 0u;
  }
}

// The body of an explicit-entries kernel: reply k from entry k, a chunk of
// kSlotBlock entries at a time, grid-strided.  Front gives the protocol's side:
//   Front::Stage          a chunk's entries in LDS
//   load(st, t, i)        entry i into stage slot t
//   word(st)              slot_rows' callable over the staged entries
template <bool FCS, class Front>
__device__ __forceinline__ void slot_frames(const Front& front, uint64_t n, const uint32_t* __restrict__ image,
                                            uint32_t* __restrict__ reply) {
  __shared__ uint32_t tab[FCS ? kRstImageDwords : 1];
  __shared__ typename Front::Stage st;
  const uint32_t t = threadIdx.x;
  if (FCS) slot_tables(tab, image);
  const auto word = front.word(st);
  for (uint64_t c0 = (uint64_t)blockIdx.x * kSlotBlock; c0 < n; c0 += (uint64_t)gridDim.x * kSlotBlock) {  // (uniform)
    const uint64_t i = c0 + t;
    __syncthreads();  // the last chunk's rows are done with st (and, first, the tables' stores)
    if (i < n) front.load(st, t, i);
    __syncthreads();
    const uint64_t left = n - c0;
    slot_rows<FCS>(tab, left < (uint64_t)kSlotBlock ? (uint32_t)left : (uint32_t)kSlotBlock, c0, reply, word);
  }
}

// A kernel's FCS form or its plain form, by the configuration's flag.
template <class... P, class... A>
inline hipError_t launch_fcs(uint32_t fcs, void (*with)(P...), void (*without)(P...), dim3 grid, dim3 block, hipStream_t stream,
                             A... args) {
  if (fcs)
    hipLaunchKernelGGL(with, grid, block, 0, stream, args...);
  else
    hipLaunchKernelGGL(without, grid, block, 0, stream, args...);
  return hipGetLastError();
}
// ... of an explicit-entries kernel (slot_frames) over n entries
template <class... P, class... A>
inline hipError_t launch_slot_frames(uint32_t fcs, void (*with)(P...), void (*without)(P...), uint64_t n, hipStream_t stream,
                                     A... args) {
  if (n == 0) return hipSuccess;
  const uint64_t chunks = (n + kSlotBlock - 1) / kSlotBlock;
  const dim3 grid((unsigned)(chunks < kSlotFramesGridCap ? chunks : kSlotFramesGridCap));
  return launch_fcs(fcs, with, without, grid, dim3(kSlotBlock), stream, args...);
}
#endif  // __HIPCC__

}  // namespace lnx
