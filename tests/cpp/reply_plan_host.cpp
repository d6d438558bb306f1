// reply_plan_host.cpp — the RST reply rules (lneto_amd/csrc/reply_plan.hpp), the
// per-frame host functions built on them (reply_host.cpp) and the table image
// that gives the FCS (table_images.cpp), compiled stand-alone for
// tests/test_rst_reply.py: no library, no GPU.  Built a second time with
// AddressSanitizer and UBSan, every frame sits in a heap block of exactly its
// length, so a field read that its length does not cover is reported: a frame
// that ends at the last byte a rule reads ends at the end of its block.
//
// Input file: u32 configs; per config lnx_rst_cfg; u32 items; per item u32 len,
// u16 ip_id, the 16 record bytes, the frame's bytes; then u32 chains; per chain
// u8 first octet, u16 seed, u32 n.  Output: a line per item, "-" for a frame
// that queues nothing, else the 20 entry bytes and the 64 slot bytes under
// every config in hex, each followed by its length; then a line per chain.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lneto_amd/csrc/reply_host.cpp"
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
  uint32_t nc = 0, ni = 0, nch = 0;
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
    lnx_tcp_rst e;
    memset(&e, 0xAA, sizeof e);
    const int rc = lnx_rx_rst_entry(frame, len, &rec, &e);
    if (rc < 0) {
      fprintf(stderr, "item %u: rc %d\n", i, rc);
      return 1;
    }
    if (rc == 0) {
      printf("-");
    } else {
      hex(&e, sizeof e);
      for (const lnx_rst_cfg& c : cfgs) {
        uint8_t* slot = static_cast<uint8_t*>(malloc(64));  // exactly the slot
        uint32_t n = 0;
        memset(slot, 0xAA, 64);
        if (lnx_tcp_rst_frame(&c, &e, ip_id, slot, &n) != LNX_OK) return 1;
        putchar(' ');
        hex(slot, 64);
        printf(" %u", n);
        free(slot);
      }
    }
    putchar('\n');
    free(frame);
  }
  must_read(&nch, 4, f);
  for (uint32_t i = 0; i < nch; ++i) {
    uint8_t first;
    uint16_t seed;
    uint32_t n;
    must_read(&first, 1, f);
    must_read(&seed, 2, f);
    must_read(&n, 4, f);
    uint16_t* out = static_cast<uint16_t*>(malloc(n ? 2 * (size_t)n : 1));  // exactly n IDs
    lnx_ip4_id_chain(first, seed, n, out);
    hex(out, 2 * (size_t)n);
    putchar('\n');
    free(out);
  }
  fclose(f);
  return 0;
}
