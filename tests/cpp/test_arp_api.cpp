// test_arp_api.cpp — include/lneto_amd.hpp's ARP mirror (arp::EntryOf, Frame,
// the batch forms' argument checks) against the built library, no GPU: the
// exchange of the reference's TestHandler (arp/arp_test.go:11-104) as the known
// answer.
#include <cstdio>
#include <cstring>
#include "lneto_amd.hpp"

#define CHECK(x)                                         \
  do {                                                   \
    if (!(x)) {                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
      return 1;                                          \
    }                                                    \
  } while (0)

int main() {
  const uint8_t hw1[6] = {0xde, 0xad, 0xbe, 0xef, 0x00, 0x00}, ip1[4] = {192, 168, 1, 1};
  const uint8_t hw2[6] = {0xc0, 0xff, 0xee, 0xc0, 0xff, 0xee}, ip2[4] = {192, 168, 1, 2};
  internet::RSTConfig c1, c2;
  memcpy(c1.MAC, hw1, 6), memcpy(c1.Addr4, ip1, 4);
  memcpy(c2.MAC, hw2, 6), memcpy(c2.Addr4, ip2, 4);

  arp::Entry q{};
  memcpy(q.ip, ip2, 4);  // StartQuery: the hardware address stays zero
  uint8_t query[64], answer[64];
  CHECK(arp::Frame(c1, arp::OpRequest, q, query) == 64);
  CHECK(query[0] == 0xFF && query[5] == 0xFF && memcmp(query + 6, hw1, 6) == 0 && query[12] == 0x08 && query[13] == 0x06);
  CHECK(query[21] == 1 && memcmp(query + 38, ip2, 4) == 0);
  CHECK(ethernet::CRC32(lneto::Bytes{query, 64}) == 0x2144DF1Cu);

  lnx_rx_delivery rec;
  CHECK(internet::Deliver(lneto::Bytes{query, 60}, 0, &rec, nullptr, nullptr) == LNX_OK);
  CHECK(rec.verdict == 0 && rec.handler == LNX_H_ETH + 8);
  arp::Entry e;
  uint8_t verdict = 0xAA;
  CHECK(arp::EntryOf(lneto::Bytes{query, 60}, rec, c2, &e, &verdict) == arp::OpRequest && verdict == 0);
  CHECK(memcmp(e.hw, hw1, 6) == 0 && memcmp(e.ip, ip1, 4) == 0 && e.zero == 0);
  CHECK(arp::EntryOf(lneto::Bytes{query, 60}, rec, c1, &e) == 0);
  CHECK(arp::EntryOf(lneto::Bytes{query, 41}, rec, c2, &e, &verdict) == 0 && verdict == 18);

  c2.AppendCRC32 = false;
  CHECK(arp::Frame(c2, arp::OpReply, e, answer) == 60 && answer[60] == 0 && answer[63] == 0);
  CHECK(memcmp(answer, hw1, 6) == 0 && memcmp(answer + 6, hw2, 6) == 0 && answer[21] == 2);
  arp::Entry seen;
  CHECK(arp::EntryOf(lneto::Bytes{answer, 60}, rec, c1, &seen) == arp::OpReply);
  CHECK(memcmp(seen.hw, hw2, 6) == 0 && memcmp(seen.ip, ip2, 4) == 0);  // CacheLookup(192.168.1.2) == c0:ff:ee:c0:ff:ee
  CHECK(arp::Frame(c2, 3, e, answer) == 0);

  // the batch forms' checks come before any device call
  CHECK(arp::Batch(nullptr, nullptr, 0, nullptr, c1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == LNX_OK);
  CHECK(arp::Batch(nullptr, nullptr, 4, nullptr, c1, 4, 4, nullptr, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(arp::FramesBatch(c1, nullptr, nullptr, 0, nullptr) == LNX_OK);
  CHECK(arp::FramesBatch(c1, nullptr, nullptr, 4, nullptr) == LNX_EINVAL);
  printf("ok\n");
  return 0;
}
