// frame_plan_host.cpp — the receive kernels' frame parse
// (lneto_amd/csrc/frame_plan.hpp) run on the host: the same rx_plan /
// rx_verdict / conv the device code inlines, with byte-pointer accessors over
// a heap copy of exactly L bytes (an accessor called outside its guard aborts,
// and is a heap overflow under -fsanitize=address) and the sums taken bytewise
// over the ranges the plan returns, in the kernels' little-endian half-word
// form at both address parities.  tests/test_frame_plan.py compares the output
// with the oracle.
//
// usage: frame_plan_host INPUT
// INPUT: u32 nfilt, nfilt x { u8 on, lnx_rx_filter }, u32 nframes, nframes x { u32 L, L bytes }
// output, one line per frame:
//   <index> <verdicts: filter-major, then flags 0..3, then address parity 0..1, 2 hex digits each>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lneto_amd/csrc/frame_plan.hpp"

namespace {

struct Frame {
  const uint8_t* b;
  uint32_t L;
  const uint8_t* at(uint32_t o, uint32_t n) const {
    if ((uint64_t)o + n > L) {
      std::fprintf(stderr, "accessor outside the frame: offset %u + %u, L = %u\n", o, n, L);
      std::abort();
    }
    return b + o;
  }
  uint32_t be16(uint32_t o) const { const uint8_t* p = at(o, 2); return (uint32_t)p[0] << 8 | p[1]; }
  uint32_t byt(uint32_t o) const { return *at(o, 1); }
  uint32_t le32(uint32_t o) const { return lnx::le32_of(at(o, 4)); }
  // the kernels' S over the frame offsets [a, b): bytes at even addresses + 256 x bytes at odd ones
  uint32_t half_sum(uint32_t mis, int32_t a, int32_t b) const {
    uint32_t s = 0;
    for (int32_t o = a; o < b; ++o) s += (uint32_t)*at((uint32_t)o, 1) << (8 * ((o + mis) & 1u));
    return s;
  }
};

uint32_t rx(const Frame& f, uint32_t mis, uint32_t flags, const lnx::RxFilter& filt) {
  auto be16 = [&](int o) { return f.be16((uint32_t)o); };
  auto byt = [&](int o) { return f.byt((uint32_t)o); };
  auto le32 = [&](int o) { return f.le32((uint32_t)o); };
  auto dyn16 = [&](uint32_t o) { return f.be16(o); };
  auto mac = [&](uint32_t& D0, uint32_t& D1) { D0 = f.le32(0), D1 = f.byt(4) | f.byt(5) << 8; };
  const lnx::RxPlan p = filt.on ? lnx::rx_plan<true>(f.L, flags, filt, be16, byt, le32, dyn16, mac)
                                : lnx::rx_plan<false>(f.L, flags, filt, be16, byt, le32, dyn16, mac);
  const uint32_t hS = p.hdr_sum ? f.half_sum(mis, 14, 34) : 0u;
  const uint32_t tS = p.l4_sum ? f.half_sum(mis, p.pa, p.pb) + f.half_sum(mis, p.la, p.lb) : 0u;
  return lnx::rx_verdict(p, lnx::conv(mis, hS), lnx::conv(mis, tS));
}

bool rd(std::FILE* in, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, in) == n; }

}  // namespace

int main(int argc, char** argv) {
  std::FILE* in = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
  if (!in) return 2;
  uint32_t nfilt = 0, nframes = 0;
  if (!rd(in, &nfilt, 4)) return 2;
  std::vector<lnx::RxFilter> filts(nfilt);
  for (auto& filt : filts) {
    uint8_t on;
    lnx_rx_filter c;
    if (!rd(in, &on, 1) || !rd(in, &c, sizeof c) || !lnx::rx_filter_of(on ? &c : nullptr, &filt)) return 2;
  }
  if (!rd(in, &nframes, 4)) return 2;
  for (uint32_t i = 0; i < nframes; ++i) {
    uint32_t L;
    if (!rd(in, &L, 4)) return 2;
    uint8_t* b = static_cast<uint8_t*>(std::malloc(L));  // exactly L bytes
    if (!rd(in, b, L)) return 2;
    std::printf("%u ", i);
    for (const auto& filt : filts)
      for (uint32_t flags = 0; flags < 4; ++flags)
        for (uint32_t mis = 0; mis < 2; ++mis) std::printf("%02x", rx(Frame{b, L}, mis, flags, filt));
    std::printf("\n");
    std::free(b);
  }
  std::fclose(in);
  return 0;
}
