// reply_kernel.hip — RST replies for SYNs to closed ports on gfx950 (DESIGN.md
// §3.19): the frame of every delivery record that queues a RST
// (reply_plan.hpp), in arrival order, one 64-byte slot a reply.
//
// Three launches on the caller's stream, none of which waits for another
// workgroup (no look-back, no grid barrier, no spin, no global atomics; the
// launches' order on the stream is the only dependency), the slice walk of
// slice_walk.hpp:
//   count  each workgroup counts the queueing frames of ONE contiguous index slice;
//   scan   over the workgroups in index order (one workgroup), and d_n;
//   build  each workgroup walks its slice again in index order, a chunk of
//          kRpBlock frames at a time: a thread per frame decides and reads the
//          frame's fields (the front end), the chunk's entries are ranked by
//          ballot / mbcnt and staged in LDS, and a 16-lane row per reply writes
//          its 16 dwords as one aligned 64-byte block (the row stage).
// lnx_tcp_rst_frames_batch is the row stage behind the other front end: the
// caller's explicit entries.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.hpp"
#include "reply_plan.hpp"
#include "slice_walk.hpp"
#include "table_layout.hpp"

namespace lnxr {

// (kRpBlock and kRpGridCap are restated in tests/test_rst_reply_gpu.py and tests/test_rst_reply_grid_mid.py)
constexpr int kRpBlock = 256;                  // frames per chunk: one per thread (tests: CHUNK)
constexpr uint32_t kRpWaves = kRpBlock / 64, kRpRows = kRpBlock / 16;
constexpr uint32_t kRpGridCap = 512;           // workgroups of the count / build launches (tests: GRID_CAP)
// ... of the explicit-entries launch, grid-strided past it (FRAMES_GRID_CAP in tests/test_rst_reply_grid_mid.py)
constexpr uint32_t kRpFramesGridCap = 2048;

// ------------------------------------------------------------------ front end: records
__device__ __forceinline__ uint32_t rp_be32(const uint8_t* a) {  // a[0..3] are all the frame's
  const uint64_t two = ((uint64_t)lnx::own_dword(a + 3) << 32) | lnx::own_dword(a);
  return __builtin_bswap32((uint32_t)(two >> (8u * (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3u))));
}

// Frame i under record i: does it queue an entry (rules 1-3)?  A frame whose
// record is not flagged costs the record's flag byte and nothing else; a flagged
// one its l4_off, its two offsets and byte 14.  p, l4: the frame's start and the
// record's l4_off, for rp_entry.
__device__ __forceinline__ bool rp_queues(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                          uint32_t trim, const uint8_t* __restrict__ rec, uint64_t i,
                                          const uint8_t*& p, uint32_t& l4) {
  const uint8_t* r = rec + 16u * i;  // lnx_rx_delivery: l4_off at 6, the ports at 8 and 10, flags at 13
  const uint32_t fl = r[13];
  if ((fl & kDlvRst) == 0) return false;
  const uint64_t s = off[i];
  const uint32_t L = lnx::frame_len(s, off[i + 1], trim);
  p = bytes + s;
  l4 = *reinterpret_cast<const uint16_t*>(r + 6);
  const uint8_t* pp = p;
  return rst_queues(L, fl, l4, [pp](uint32_t o) -> uint32_t { return lnx::own_byte(pp + o); });
}

// ------------------------------------------------------------------ count, scan
__global__ void __launch_bounds__(kRpBlock)
rst_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint8_t* __restrict__ rec, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kRpWaves];
  uint64_t lo, hi;
  lnx::slice_bounds(n, kRpBlock, lo, hi);
  uint32_t c = 0;
  for (uint64_t c0 = lo; c0 < hi; c0 += kRpBlock) {  // (uniform)
    const uint64_t i = c0 + threadIdx.x;
    const uint8_t* p = bytes;
    uint32_t l4 = 0;
    if (i < hi && rp_queues(bytes, off, trim, rec, i, p, l4)) c += 1u;
  }
  c = lnx::wave_add(c);
  if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < kRpWaves; ++w) s += wsum[w];
    counts[blockIdx.x] = s;
  }
}

// counts[g] becomes the queueing frames in the workgroups before g; d_n = {written, wanted}
__global__ void __launch_bounds__(kRpGridCap)
rst_scan_kernel(uint32_t* __restrict__ counts, uint32_t G, uint64_t cap, uint32_t* __restrict__ d_n) {
  __shared__ uint32_t part[kRpGridCap];
  const uint32_t t = threadIdx.x;
  const uint32_t c = t < G ? counts[t] : 0u;
  const uint32_t inc = lnx::block_scan_inclusive<kRpGridCap>(part, c);
  if (t < G) counts[t] = inc - c;
  if (t == G - 1u) {  // the last workgroup's inclusive sum: the total
    const uint32_t total = inc;  // (n < 2^32)
    d_n[0] = total < cap ? total : (uint32_t)cap;
    d_n[1] = total;
  }
}

// ------------------------------------------------------------------ the row stage
// A chunk's entries in LDS, by rank: the address, remote | local << 16, seq, ack, flags | IP ID << 16.
struct RpStage {
  uint32_t addr[kRpBlock], ports[kRpBlock], seq[kRpBlock], ack[kRpBlock], flid[kRpBlock];
};

// Replies k0 .. k0 + m - 1 from the staged entries 0 .. m - 1: row `row` takes
// entries row, row + 16, ...; lane p of the row makes dword p (reply_plan.hpp
// rst_word; every lane takes the two sums, a handful of adds), the row XORs the
// fifteen shares of the FCS and lane 15 holds its complement.  The row's sixteen
// stores are one whole aligned 64-byte block.
template <bool FCS>
__device__ __forceinline__ void rp_rows(const RpStage& st, const uint32_t* tab, uint32_t m, uint64_t k0,
                                        const RstCfg& cfg, uint32_t* __restrict__ reply) {
  const uint32_t p = threadIdx.x & 15u, row = threadIdx.x >> 4;
  const uint32_t pw = p < lnx::kRstLanes ? p : lnx::kRstLanes - 1u;
  const uint32_t fixed = rst_fixed_word(pw, cfg);
  for (uint32_t j0 = 0; j0 < m; j0 += kRpRows) {  // (uniform: m <= kRpBlock, so j < kRpBlock; a row past m stores nothing)
    const uint32_t j = j0 + row;
    RstEntry e;
    e.addr = st.addr[j];
    e.remote_port = st.ports[j] & 0xFFFFu, e.local_port = st.ports[j] >> 16;
    e.seq = st.seq[j], e.ack = st.ack[j];
    e.flags = st.flid[j] & 0xFFFFu;
    const uint32_t id = st.flid[j] >> 16;
    const uint32_t ip_sum = rst_ip_sum(cfg, e, id), tcp_sum = rst_tcp_sum(cfg, e);
    uint32_t w = rst_word(pw, fixed, e, id, ip_sum, tcp_sum);
    if (FCS) {
      uint32_t z = rst_fcs_part(pw, w, [tab](uint32_t q, uint32_t i, uint32_t v) -> uint32_t { return tab[lnx::rst_nib(q, i, v)]; });
      z = lnx::row_xor16(p < lnx::kRstLanes ? z : 0u);
      w = p < lnx::kRstLanes ? w : ~z;
    } else {
      w = p < lnx::kRstLanes ? w : 0u;
    }
    if (j < m) reply[(k0 + j) * kRstWords + p] = w;
  }
}

__device__ __forceinline__ void rp_tables(uint32_t* tab, const uint32_t* __restrict__ image) {
  for (uint32_t i = threadIdx.x; i < lnx::kRstImageDwords; i += kRpBlock) tab[i] = image[lnx::kRstImgZ + i];
}

// ------------------------------------------------------------------ build
// run: the queueing frames before the chunk (the scan's base of this workgroup,
// then the chunks walked).  A frame's rank in its chunk: the waves' counts
// before its wave (through LDS) plus the queueing lanes below it in its wave.
// Nothing at or past `cap` is written: no slot, no d_src entry, and no ID is read.
template <bool FCS>
__global__ void __launch_bounds__(kRpBlock)
rst_reply_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint8_t* __restrict__ rec, RstCfg cfg, const uint16_t* __restrict__ ip_id, uint64_t cap,
                 const uint32_t* __restrict__ base, const uint32_t* __restrict__ image, uint32_t* __restrict__ reply,
                 uint32_t* __restrict__ src) {
  __shared__ uint32_t tab[lnx::kRstImageDwords];
  __shared__ RpStage st;
  __shared__ uint32_t wcnt[kRpWaves];
  const uint32_t t = threadIdx.x, wave = t >> 6;
  rp_tables(tab, image);
  uint64_t lo, hi;
  lnx::slice_bounds(n, kRpBlock, lo, hi);
  uint64_t run = base[blockIdx.x];
  for (uint64_t c0 = lo; c0 < hi && run < cap; c0 += kRpBlock) {  // (uniform: every wave keeps all its lanes)
    const uint64_t i = c0 + t;
    const uint8_t* p = bytes;
    uint32_t l4 = 0;
    const bool q = i < hi && rp_queues(bytes, off, trim, rec, i, p, l4);
    uint32_t below, wq;
    lnx::wave_rank(q, below, wq);
    __syncthreads();  // the last chunk's rows are done with st and wcnt (and, first, the tables' stores)
    if ((t & 63u) == 0) wcnt[wave] = wq;
    __syncthreads();
    uint32_t before, total;
    lnx::waves_before<kRpWaves>(wcnt, wave, before, total);
    const uint32_t r = before + below;  // < kRpBlock
    if (q && run + r < cap) {
      const uint8_t* pp = p;
      const uint32_t ports = *reinterpret_cast<const uint32_t*>(rec + 16u * i + 8);  // src_port | dst_port << 16
      const RstEntry e = rst_entry_of(l4, ports & 0xFFFFu, ports >> 16, [pp](uint32_t o) -> uint32_t { return rp_be32(pp + o); });
      st.addr[r] = e.addr;
      st.ports[r] = e.remote_port | (e.local_port << 16);
      st.seq[r] = e.seq;
      st.ack[r] = e.ack;
      st.flid[r] = e.flags | ((uint32_t)ip_id[run + r] << 16);
      src[run + r] = (uint32_t)i;
    }
    __syncthreads();
    const uint64_t room = cap - run;
    rp_rows<FCS>(st, tab, total < room ? total : (uint32_t)room, run, cfg, reply);
    run += total;
  }
}

// ------------------------------------------------------------------ front end: explicit entries
// entry: lnx_tcp_rst as five little-endian dwords (the address bytes, remote |
// local << 16, seq, ack, flags | zero << 16); reply k from entry k.
template <bool FCS>
__global__ void __launch_bounds__(kRpBlock)
rst_frames_kernel(const uint32_t* __restrict__ entry, uint64_t n, RstCfg cfg, const uint16_t* __restrict__ ip_id,
                  const uint32_t* __restrict__ image, uint32_t* __restrict__ reply) {
  __shared__ uint32_t tab[lnx::kRstImageDwords];
  __shared__ RpStage st;
  const uint32_t t = threadIdx.x;
  rp_tables(tab, image);
  for (uint64_t c0 = (uint64_t)blockIdx.x * kRpBlock; c0 < n; c0 += (uint64_t)gridDim.x * kRpBlock) {  // (uniform)
    const uint64_t i = c0 + t;
    __syncthreads();  // the last chunk's rows are done with st (and, first, the tables' stores)
    if (i < n) {
      const uint32_t* w = entry + 5u * i;
      st.addr[t] = __builtin_bswap32(w[0]);
      st.ports[t] = w[1];
      st.seq[t] = w[2];
      st.ack[t] = w[3];
      st.flid[t] = (w[4] & 0xFFFFu) | ((uint32_t)ip_id[i] << 16);
    }
    __syncthreads();
    const uint64_t left = n - c0;
    rp_rows<FCS>(st, tab, left < (uint64_t)kRpBlock ? (uint32_t)left : (uint32_t)kRpBlock, c0, cfg, reply);
  }
}

// ------------------------------------------------------------------ launchers
// ws: the workgroups' counts, then bases (G words)
uint64_t rst_ws_bytes(uint64_t n) { return (uint64_t)lnx::slice_grid(n, kRpBlock, kRpGridCap) * 4u; }

// n > 0.  cap == 0: d_n alone is written (count and scan).
hipError_t launch_rst_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                            const lnx_rst_cfg& cfg, const uint16_t* ip_id, uint64_t cap, uint8_t* reply, uint32_t* src,
                            uint32_t* d_n, void* ws, const uint32_t* image, hipStream_t stream) {
  const uint32_t G = lnx::slice_grid(n, kRpBlock, kRpGridCap);
  const RstCfg c = rst_cfg_of(cfg);
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(rec);
  uint32_t* counts = static_cast<uint32_t*>(ws);
  hipError_t e;
  hipLaunchKernelGGL(rst_count_kernel, dim3(G), dim3(kRpBlock), 0, stream, bytes, off, n, trim, rb, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(rst_scan_kernel, dim3(1), dim3(kRpGridCap), 0, stream, counts, G, cap, d_n);
  if ((e = hipGetLastError()) != hipSuccess || cap == 0) return e;
  uint32_t* out = reinterpret_cast<uint32_t*>(reply);
  if (c.fcs)
    hipLaunchKernelGGL(rst_reply_kernel<true>, dim3(G), dim3(kRpBlock), 0, stream, bytes, off, n, trim, rb, c, ip_id, cap,
                       counts, image, out, src);
  else
    hipLaunchKernelGGL(rst_reply_kernel<false>, dim3(G), dim3(kRpBlock), 0, stream, bytes, off, n, trim, rb, c, ip_id, cap,
                       counts, image, out, src);
  return hipGetLastError();
}

hipError_t launch_rst_frames(const lnx_rst_cfg& cfg, const lnx_tcp_rst* entry, uint64_t n, const uint16_t* ip_id,
                             uint8_t* reply, const uint32_t* image, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const RstCfg c = rst_cfg_of(cfg);
  const uint64_t chunks = (n + kRpBlock - 1) / kRpBlock;
  const dim3 grid((unsigned)(chunks < kRpFramesGridCap ? chunks : kRpFramesGridCap));
  const uint32_t* in = reinterpret_cast<const uint32_t*>(entry);
  uint32_t* out = reinterpret_cast<uint32_t*>(reply);
  if (c.fcs)
    hipLaunchKernelGGL(rst_frames_kernel<true>, grid, dim3(kRpBlock), 0, stream, in, n, c, ip_id, image, out);
  else
    hipLaunchKernelGGL(rst_frames_kernel<false>, grid, dim3(kRpBlock), 0, stream, in, n, c, ip_id, image, out);
  return hipGetLastError();
}

}  // namespace lnxr
