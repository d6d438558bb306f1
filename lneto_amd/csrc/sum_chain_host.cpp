// sum_chain_host.cpp — the running forms of the internet checksum on the host
// (lneto CRC791, crc.go:13-62): the raw 32-bit sum of a piece at either byte
// phase of its packet, and PayloadSum16 over a frame held in several buffers.
// No HIP and no other source of the library: tests/cpp/sum_chain_host_main.cpp
// compiles this file alone.
//
// With E = the sum of a piece's bytes at even offsets from its own start and
// O = the sum of those at odd offsets (both mod 2^32), the reference's 32-bit
// value before sum16 (crc.go:17-21) over seed s and bytes B is
//   S(s, B) = s + 256 E + O   (mod 2^32)
// — sumWriteEven's big-endian words (crc.go:23-28) and the `<< 8` of an odd
// last byte (crc.go:56).  A piece that starts at an odd offset of its packet
// has the two weights swapped.  Everything is linear mod 2^32, so the
// reference's own wrap-around (carries lost on long data) is reproduced
// exactly; a 64-bit accumulator or an end-around carry before the last step
// would not be.
#include <cstddef>
#include <cstdint>
#include "../../include/lneto_amd.h"

extern "C" {

uint32_t lnx_sum_partial(uint32_t sum, const uint8_t* p, size_t n, int phase) {
  uint32_t e = 0, o = 0;
  size_t i = 0;
  for (; i + 1 < n; i += 2) e += p[i], o += p[i + 1];
  if (i < n) e += p[i];
  return (phase & 1) ? sum + e + 256u * o : sum + 256u * e + o;
}

uint16_t lnx_sum16_chain(uint32_t seed, const uint8_t* const* seg, const size_t* len, size_t m) {
  uint32_t sum = seed;
  int phase = 0;  // only the parity of the bytes so far matters: no byte count to overflow
  for (size_t k = 0; k < m; ++k) {
    if (len[k] == 0) continue;  // an empty segment's pointer is never read
    sum = lnx_sum_partial(sum, seg[k], len[k], phase);
    phase ^= (int)(len[k] & 1u);
  }
  sum = (sum & 0xffffu) + (sum >> 16);  // sum16, crc.go:17-21
  return (uint16_t)~(uint16_t)(sum + (sum >> 16));
}

}  // extern "C"
