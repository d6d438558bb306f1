// The running-checksum delegates of include/lneto_amd.hpp against the built
// library (tests/test_sum_chain.py): CRC791::WritePartial, PayloadSum16Chain
// and the two batch delegates' argument checks, none of which touches a GPU.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "lneto_amd.hpp"

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);          \
      ++failures;                                               \
    }                                                           \
  } while (0)

int main() {
  std::vector<uint8_t> hdr(21), pay(1461);
  for (size_t i = 0; i < hdr.size(); ++i) hdr[i] = (uint8_t)(0x45 + 7 * i);
  for (size_t i = 0; i < pay.size(); ++i) pay[i] = (uint8_t)(i * 131 + 9);
  std::vector<uint8_t> all(hdr);
  all.insert(all.end(), pay.begin(), pay.end());

  lneto::CRC791 whole, parts;
  whole.AddUint32(0xC0A80A01u);
  parts.AddUint32(0xC0A80A01u);
  const uint16_t want = whole.PayloadSum16(all);
  parts.WritePartial(hdr);                         // 21 bytes: the payload starts at an odd offset
  parts.WritePartial(pay, (int)(hdr.size() & 1));
  CHECK(parts.Sum16() == want);

  const uint8_t* seg[2] = {hdr.data(), pay.data()};
  const size_t len[2] = {hdr.size(), pay.size()};
  CHECK(lneto::PayloadSum16Chain(whole.sum, seg, len, 2) == want);
  CHECK(lneto::PayloadSum16Chain(whole.sum, seg, len, 0) == whole.Sum16());

  // a cached payload sum under a rewritten header: the payload's raw sum is the header's seed
  lneto::CRC791 cached;
  cached.WritePartial(pay, 1);
  hdr[3] ^= 0x40;
  lneto::CRC791 again;
  again.sum = cached.sum;
  again.WritePartial(hdr);
  std::vector<uint8_t> all2(hdr);
  all2.insert(all2.end(), pay.begin(), pay.end());
  CHECK(again.Sum16() == lneto::CRC791{}.PayloadSum16(all2));

  // the batch delegates: a zero count is a no-op, NULL pointers with a count are LNX_EINVAL
  uint32_t buf[16] = {};
  auto* p8 = reinterpret_cast<const uint8_t*>(buf);
  auto* p64 = reinterpret_cast<const uint64_t*>(buf);
  CHECK(lneto::SumPartialBatch(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == LNX_OK);
  CHECK(lneto::SumPartialBatch(nullptr, p64, buf, nullptr, nullptr, 4, buf) == LNX_EINVAL);
  CHECK(lneto::SumPartialBatch(p8, p64, buf, buf, nullptr, 4, buf + 3) == LNX_EINVAL);  // d_seed overlaps d_sum
  CHECK(lneto::PayloadSum16ChainBatch(nullptr, nullptr, nullptr, 3, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == LNX_OK);
  CHECK(lneto::PayloadSum16ChainBatch(p8, p64, buf, 2, p64, 2, nullptr, buf, nullptr, nullptr) == LNX_EINVAL);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
