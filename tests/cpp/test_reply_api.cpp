// test_reply_api.cpp — include/lneto_amd.hpp's RST reply mirror (internet::
// RSTConfig, RSTEntryOf, RSTFrame, IPIDChain, the batch forms' argument checks)
// against the built library, no GPU: TestStackPorts_RSTOnUnknownPort's frame
// (internet/tcplistener_test.go:458-527) as the known answer.
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
  uint8_t f[54] = {};
  f[12] = 0x08;
  f[14] = 0x45, f[23] = 6;
  f[17] = 40;
  const uint8_t client[4] = {10, 0, 0, 1}, server[4] = {10, 0, 0, 2};
  memcpy(f + 26, client, 4), memcpy(f + 30, server, 4);
  f[34] = 5000 >> 8, f[35] = 5000 & 255, f[36] = 443 >> 8, f[37] = 443 & 255;
  f[40] = 700 >> 8, f[41] = 700 & 255;  // seq 700
  f[46] = 0x50, f[47] = 0x02;           // SYN
  internet::StackPortTables ports;
  ports.TCP = {80};
  lnx_rx_delivery rec;
  CHECK(internet::Deliver(lneto::Bytes{f, sizeof f}, 0, &rec, nullptr, &ports) == LNX_OK);
  CHECK(rec.verdict == 2 && (rec.flags & LNX_DLV_RST));
  tcp::RSTEntry e;
  CHECK(internet::RSTEntryOf(lneto::Bytes{f, sizeof f}, rec, &e));
  CHECK(e.remote_port == 5000 && e.local_port == 443 && e.seq == 0 && e.ack == 701);
  CHECK(e.flags == (tcp::FlagRST | tcp::FlagACK) && memcmp(e.remote_addr, client, 4) == 0);
  CHECK(!internet::RSTEntryOf(lneto::Bytes{f, 29}, rec, &e));

  internet::RSTConfig cfg;
  memcpy(cfg.Addr4, server, 4);
  cfg.MAC[5] = 1, cfg.GatewayMAC[5] = 2;
  uint16_t ids[3];
  internet::IPIDChain(cfg.Addr4[0], 0, 3, ids);
  uint8_t out[64];
  CHECK(internet::RSTFrame(cfg, e, ids[0], out) == 64);
  CHECK(out[5] == 2 && out[11] == 1 && out[12] == 0x08 && out[13] == 0x00 && out[14] == 0x45 && out[17] == 40);
  CHECK(out[18] == (ids[0] >> 8) && out[19] == (ids[0] & 255) && out[20] == 0x40 && out[22] == 64 && out[23] == 6);
  CHECK(memcmp(out + 26, server, 4) == 0 && memcmp(out + 30, client, 4) == 0);
  CHECK(out[34] == (443 >> 8) && out[35] == (443 & 255) && out[36] == (5000 >> 8) && out[37] == (5000 & 255));
  CHECK(out[44] == (701 >> 8) && out[45] == (701 & 255) && out[46] == 0x50 && out[47] == 0x14);
  CHECK(ethernet::CRC32(lneto::Bytes{out, 64}) == 0x2144DF1Cu);
  cfg.AppendCRC32 = false;
  CHECK(internet::RSTFrame(cfg, e, ids[0], out) == 60 && out[60] == 0 && out[63] == 0);

  // the batch forms' checks come before any device call
  CHECK(internet::RSTReplyBatch(nullptr, nullptr, 0, nullptr, cfg, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == LNX_OK);
  CHECK(internet::RSTReplyBatch(nullptr, nullptr, 4, nullptr, cfg, nullptr, 4, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(internet::RSTFramesBatch(cfg, nullptr, 0, nullptr, nullptr) == LNX_OK);
  CHECK(internet::RSTFramesBatch(cfg, nullptr, 4, nullptr, nullptr) == LNX_EINVAL);
  printf("ok\n");
  return 0;
}
