// deliver_plan_host.cpp — the delivery rules (lneto_amd/csrc/deliver_plan.hpp)
// and the per-frame host function built on them (deliver_host.cpp), compiled
// stand-alone for tests/test_deliver.py: no library, no GPU.  Built a second
// time with AddressSanitizer and UBSan, every frame sits in a heap block of
// exactly its length, so a field read that its length does not cover is
// reported.
//
// Input file: u32 settings; per setting u8 has_filter, lnx_rx_filter,
// u8 has_ports, lnx_rx_ports; u32 frames; per frame u32 len, u8 verdict_in,
// i8 fcs_ok (< 0: none), the bytes.  Output: a line per frame, the 16 record
// bytes of every setting in hex.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lneto_amd/csrc/deliver_host.cpp"

struct Setting {
  bool has_filter, has_ports;
  lnx_rx_filter filter;
  lnx_rx_ports ports;
};

static void must_read(void* p, size_t n, FILE* f) {
  if (n && fread(p, 1, n, f) != n) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t ns = 0, nf = 0;
  must_read(&ns, 4, f);
  std::vector<Setting> settings(ns);
  for (Setting& s : settings) {
    uint8_t b;
    must_read(&b, 1, f);
    s.has_filter = b != 0;
    must_read(&s.filter, sizeof s.filter, f);
    must_read(&b, 1, f);
    s.has_ports = b != 0;
    must_read(&s.ports, sizeof s.ports, f);
  }
  must_read(&nf, 4, f);
  for (uint32_t i = 0; i < nf; ++i) {
    uint32_t len;
    uint8_t v_in;
    int8_t fcs;
    must_read(&len, 4, f);
    must_read(&v_in, 1, f);
    must_read(&fcs, 1, f);
    uint8_t* frame = len ? static_cast<uint8_t*>(malloc(len)) : nullptr;  // exactly the frame
    must_read(frame, len, f);
    for (const Setting& s : settings) {
      lnx_rx_delivery d;
      memset(&d, 0xAA, sizeof d);
      const int rc = lnx_rx_deliver(frame, len, s.has_filter ? &s.filter : nullptr, s.has_ports ? &s.ports : nullptr, fcs,
                                    v_in, &d);
      if (rc != LNX_OK) {
        fprintf(stderr, "frame %u: rc %d\n", i, rc);
        return 1;
      }
      const uint8_t* raw = reinterpret_cast<const uint8_t*>(&d);
      for (size_t k = 0; k < sizeof d; ++k) printf("%02x", raw[k]);
      putchar(' ');
    }
    putchar('\n');
    free(frame);
  }
  fclose(f);
  return 0;
}
