// arp_plan_host.cpp — the ARP rules (lneto_amd/csrc/arp_plan.hpp), the per-frame
// host functions built on them (arp_host.cpp) and the table image that gives
// the FCS (table_images.cpp), compiled stand-alone for tests/test_arp_reply.py:
// no library, no GPU.  Built a second time with AddressSanitizer and UBSan,
// every frame sits in a heap block of exactly its length, so a field read that
// its length does not cover is reported: a frame that ends at the last byte a
// rule reads ends at the end of its block.
//
// Input file: u32 configs; per config lnx_rst_cfg; u32 items; per item u32 len,
// the 16 record bytes, the frame's bytes.  Output: a line per item and config,
// "kind verdict", and for kinds 1 and 2 the 12 entry bytes and the 64 slot
// bytes of the frame for op 2 and for op 1 in hex, each followed by its length.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lneto_amd/csrc/arp_host.cpp"
#include "../../lneto_amd/csrc/table_images.cpp"

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
    lnx_rx_delivery rec;
    must_read(&len, 4, f);
    must_read(&rec, sizeof rec, f);
    uint8_t* frame = len ? static_cast<uint8_t*>(malloc(len)) : nullptr;  // exactly the frame
    must_read(frame, len, f);
    for (const lnx_rst_cfg& c : cfgs) {
      lnx_arp_entry e;
      uint8_t verdict = 0xAA;
      memset(&e, 0xAA, sizeof e);
      const int kind = lnx_rx_arp_entry(frame, len, &rec, &c, &e, &verdict);
      if (kind < 0) {
        fprintf(stderr, "item %u: rc %d\n", i, kind);
        return 1;
      }
      printf("%d %u", kind, (unsigned)verdict);
      if (kind != 0) {
        putchar(' ');
        hex(&e, sizeof e);
        for (uint16_t op = 2; op >= 1; --op) {
          uint8_t* slot = static_cast<uint8_t*>(malloc(64));  // exactly the slot
          uint32_t n = 0;
          memset(slot, 0xAA, 64);
          if (lnx_arp_frame(&c, op, &e, slot, &n) != LNX_OK) return 1;
          putchar(' ');
          hex(slot, 64);
          printf(" %u", n);
          free(slot);
        }
      }
      putchar('\n');
    }
    free(frame);
  }
  fclose(f);
  return 0;
}
