// echo_plan_host.cpp — the echo reply rules (lneto_amd/csrc/echo_plan.hpp) and
// the per-frame host functions built on them (echo_host.cpp), compiled
// stand-alone for tests/test_echo_reply.py: no library, no GPU.  Built a second
// time with AddressSanitizer and UBSan, every frame sits in a heap block of
// exactly its length and every reply in one of exactly the length the function
// reports, so a read that the frame's length does not cover, or a write past
// *len, is reported: a frame whose data ends at its last byte ends at the end of
// its block.
//
// Input file: u32 configs; per config lnx_rst_cfg; u32 items; per item u32 len,
// u16 ip_id, the 16 record bytes, the frame's bytes.  Output: a line per item,
// "-" for a frame that queues nothing, else the 16 entry bytes in hex and, under
// every config, the reply's first 64 bytes in hex, the CRC-32 of the whole
// reply, its length, and what a buffer one byte short returns.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lneto_amd/csrc/echo_host.cpp"

static void must_read(void* p, size_t n, FILE* f) {
  if (n && fread(p, 1, n, f) != n) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}
static void hex(const void* p, size_t n) {
  const uint8_t* raw = static_cast<const uint8_t*>(p);
  for (size_t k = 0; k < n; ++k) printf("%02x", raw[k]);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t nc = 0, ni = 0;
  must_read(&nc, 4, f);
  std::vector<lnx_rst_cfg> cfgs(nc);
  for (lnx_rst_cfg& c : cfgs) must_read(&c, sizeof c, f);
  must_read(&ni, 4, f);
  for (uint32_t i = 0; i < ni; ++i) {
    uint32_t len;
    uint16_t ip_id;
    lnx_rx_delivery rec;
    must_read(&len, 4, f);
    must_read(&ip_id, 2, f);
    must_read(&rec, sizeof rec, f);
    uint8_t* frame = len ? static_cast<uint8_t*>(malloc(len)) : nullptr;  // exactly the frame
    must_read(frame, len, f);
    lnx_icmp_echo e;
    memset(&e, 0xAA, sizeof e);
    const int rc = lnx_rx_echo_entry(frame, len, &rec, &e);
    if (rc < 0) {
      fprintf(stderr, "item %u: rc %d\n", i, rc);
      return 1;
    }
    if (rc == 0) {
      printf("-");
    } else {
      hex(&e, sizeof e);
      for (const lnx_rst_cfg& c : cfgs) {
        const uint32_t want = lnxe::echo_len(e.data_len, c.flags & LNX_TX_FCS);
        uint8_t* out = static_cast<uint8_t*>(malloc(want));  // exactly the reply
        uint32_t n = 0;
        memset(out, 0xAA, want);
        if (lnx_icmp_echo_reply_frame(&c, &e, frame + e.data_off, ip_id, out, want, &n) != LNX_OK || n != want) return 1;
        uint32_t reg = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < n; ++k) reg = lnxe::echo_crc_byte(reg, out[k]);
        putchar(' ');
        hex(out, n < 64 ? n : 64);
        printf(" %08x %u", ~reg, n);
        uint8_t* small = static_cast<uint8_t*>(malloc(want - 1));  // one byte short: nothing may be written
        printf(" %d", lnx_icmp_echo_reply_frame(&c, &e, frame + e.data_off, ip_id, small, want - 1, &n));
        free(small);
        free(out);
      }
    }
    putchar('\n');
    free(frame);
  }
  fclose(f);
  return 0;
}
