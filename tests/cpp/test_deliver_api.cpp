// test_deliver_api.cpp — include/lneto_amd.hpp's receive delivery mirror
// (internet::StackPortTables, Deliver, DeliverBatch) against the built library,
// on the host: a SYN to a listening port, to a closed one, a datagram, and the
// argument errors of the batch entry, which need no device.
#include <cstdio>
#include <vector>
#include "lneto_amd.hpp"

static int fails = 0;
#define CHECK(c)                                        \
  do {                                                  \
    if (!(c)) {                                         \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                          \
    }                                                   \
  } while (0)

// Ethernet + IPv4 (IHL 5) + the first 20 bytes of a TCP header / 8 of a UDP
// header; the checksums are not looked at here (the verdict is an input)
static std::vector<uint8_t> frame4(uint8_t proto, uint16_t sport, uint16_t dport, uint16_t tcp_flags) {
  const size_t l4 = proto == 6 ? 20 : 8;
  std::vector<uint8_t> f(14 + 20 + l4, 0);
  f[12] = 0x08;
  f[14] = 0x45;
  f[16] = uint8_t((20 + l4) >> 8), f[17] = uint8_t(20 + l4);
  f[23] = proto;
  f[34] = uint8_t(sport >> 8), f[35] = uint8_t(sport);
  f[36] = uint8_t(dport >> 8), f[37] = uint8_t(dport);
  if (proto == 6) f[46] = uint8_t(0x50 | (tcp_flags >> 8)), f[47] = uint8_t(tcp_flags);
  return f;
}

int main() {
  internet::StackPortTables ports;
  ports.TCP = {22, 80, 80};
  ports.UDP = {53};
  internet::StackFilter filt;
  lnx_rx_delivery d;

  CHECK(internet::Deliver(frame4(6, 40000, 80, 0x002), 0, &d, &filt, &ports) == LNX_OK);
  CHECK(d.handler == LNX_H_TCP + 1 && d.verdict == 0 && d.flags == 0 && d.l4_off == 34 && d.ip_end == 54);
  CHECK(d.src_port == 40000 && d.dst_port == 80 && d.zero == 0);
  CHECK(internet::Deliver(frame4(6, 40000, 81, 0x002), 0, &d, &filt, &ports) == LNX_OK);
  CHECK(d.handler == LNX_H_NONE && d.verdict == 2 && d.flags == LNX_DLV_RST && d.dst_port == 81);
  CHECK(internet::Deliver(frame4(6, 40000, 81, 0x012), 0, &d, &filt, &ports) == LNX_OK);
  CHECK(d.handler == LNX_H_NONE && d.verdict == 2 && d.flags == 0);
  for (uint16_t fl : {0x000, 0x001, 0x008}) {  // no SYN (and no RST, no ACK): dropped without a RST
    CHECK(internet::Deliver(frame4(6, 40000, 81, fl), 0, &d, &filt, &ports) == LNX_OK);
    CHECK(d.handler == LNX_H_NONE && d.verdict == 2 && d.flags == 0 && d.dst_port == 81);
  }
  CHECK(internet::Deliver(frame4(17, 40000, 53, 0), 0, &d, &filt, &ports) == LNX_OK);
  CHECK(d.handler == LNX_H_UDP + 0 && d.verdict == 0 && d.ip_end == 42);
  CHECK(internet::Deliver(frame4(17, 40000, 54, 0), 0, &d) == LNX_OK);  // no tables: every port has a handler
  CHECK(d.handler == LNX_H_UDP + 256);
  CHECK(internet::Deliver(frame4(17, 40000, 53, 0), 3, &d, &filt, &ports) == LNX_OK);
  CHECK(d.handler == LNX_H_NONE && d.verdict == 3 && d.dst_port == 0);
  CHECK(internet::Deliver(frame4(17, 40000, 53, 0), 0, &d, &filt, &ports, 0) == LNX_OK);
  CHECK(d.verdict == 3 && d.flags == LNX_DLV_FCS);
  std::vector<uint8_t> cut = frame4(6, 40000, 80, 0x002);
  cut.resize(40);
  CHECK(internet::Deliver(cut, 0, &d, &filt, &ports) == LNX_OK);
  CHECK(d.verdict == 18 && d.handler == LNX_H_NONE && d.ip_end == 0);

  internet::StackPortTables many;
  many.TCP.assign(257, 1);
  CHECK(internet::Deliver(frame4(6, 1, 1, 2), 0, &d, nullptr, &many) == LNX_EINVAL);
  alignas(16) static uint8_t mem[64];
  const uint8_t* b = mem;
  const uint64_t* off = reinterpret_cast<const uint64_t*>(mem);
  lnx_rx_delivery* rec = reinterpret_cast<lnx_rx_delivery*>(mem);
  uint32_t* w = reinterpret_cast<uint32_t*>(mem);
  CHECK(internet::DeliverBatch(b, off, 1, nullptr, b, rec, w, nullptr, mem) == LNX_EINVAL);   // d_count alone missing
  CHECK(internet::DeliverBatch(b, off, 1, nullptr, b, rec, nullptr, w, mem) == LNX_EINVAL);
  CHECK(internet::DeliverBatch(b, off, uint64_t(1) << 32, nullptr, b, rec) == LNX_EINVAL);
  CHECK(internet::DeliverBatch(b, off, 1, nullptr, b, rec, nullptr, nullptr, nullptr, nullptr, &many) == LNX_EINVAL);
  CHECK(internet::DeliverBatch(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == LNX_OK);
  CHECK(lnx_rx_deliver_ws_bytes(1) == 4 * (LNX_H_COUNT + 1) + 2);
  if (fails == 0) std::printf("ok\n");
  return fails != 0;
}
