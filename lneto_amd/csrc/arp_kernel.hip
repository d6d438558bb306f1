// arp_kernel.hip — ARP on gfx950: the reply of every ARP
// request for our address and the learn record of every ARP reply
// (arp_plan.hpp), in arrival order, one 64-byte slot a reply and one 16-byte
// record a learned sender.
//
// Three launches on the caller's stream, none of which waits for another
// workgroup (no look-back, no grid barrier, no spin, no global atomics; the
// launches' order on the stream is the only dependency), the slice walk of
// slice_walk.hpp:
//   count  each workgroup counts the requests for us (kind 1) and the replies
//          (kind 2) of ONE contiguous index slice;
//   scan   over the workgroups in index order (one workgroup): the two running
//          sums in the same rounds, and d_n;
//   build  each workgroup walks its slice again in index order, a chunk of
//          kArBlock frames at a time: a thread per frame decides (the front
//          end) and is ranked once per kind by ballot / mbcnt; a kind-2 thread
//          stores its own record; the chunk's kind-1 entries are staged in LDS
//          by rank, and a 16-lane row per reply writes its 16 dwords as one
//          aligned 64-byte block (the row stage of §3.19, with the FCS from the
//          kRstImgZ tables).
// lnx_arp_frames_batch is the row stage behind the other front end: the
// caller's explicit entries and ops.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "arp_plan.hpp"
#include "launch.hpp"
#include "slice_walk.hpp"
#include "table_layout.hpp"

namespace lnxa {

// (kArBlock, kArGridCap and kArFramesGridCap are restated in tests/test_arp_reply_gpu.py)
constexpr int kArBlock = 256;                  // frames per chunk: one per thread (tests: CHUNK)
constexpr uint32_t kArWaves = kArBlock / 64, kArRows = kArBlock / 16;
constexpr uint32_t kArGridCap = 512;           // workgroups of the count / build launches (tests: GRID_CAP)
constexpr uint32_t kArFramesGridCap = 2048;    // ... of the explicit-entries launch, grid-strided past it (tests: FRAMES_GRID_CAP)

// ------------------------------------------------------------------ front end: records
// Frame bytes 14 .. 41, the ARP body, as seven little-endian dwords.  Eight
// aligned loads issued back to back, each of a dword that holds one of those
// bytes: at phase 0 the eighth would lie past byte 41, and takes the seventh again.
struct ArBody {
  uint32_t w[kArpV4 / 4];
};
__device__ __forceinline__ ArBody ar_body(const uint8_t* p) {  // L >= 42
  const uintptr_t a = reinterpret_cast<uintptr_t>(p + kArpBody), al = a & ~(uintptr_t)3;
  const uint32_t sh = 8u * (uint32_t)(a & 3u);
  uint32_t d[kArpV4 / 4 + 1];
#pragma unroll
  for (uint32_t k = 0; k < kArpV4 / 4; ++k) d[k] = *reinterpret_cast<const uint32_t*>(al + 4u * k);
  d[kArpV4 / 4] = *reinterpret_cast<const uint32_t*>(al + (sh ? kArpV4 : kArpV4 - 4u));
  ArBody b;
#pragma unroll
  for (uint32_t k = 0; k < kArpV4 / 4; ++k) b.w[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> sh);
  return b;
}

// Frame i under record i: its kind (arp_plan.hpp), and for kinds 1 and 2 the
// sender in e.  A frame whose record rules it out costs its 16-byte record
// alone, one dwordx4; a candidate its two offsets and bytes 12 .. 13, and one
// of at least 42 bytes bytes 14 .. 41, all from the frame's own aligned dwords.
__device__ __forceinline__ uint32_t ar_kind(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                            uint32_t trim, const uint4* __restrict__ rec, uint64_t i, const ArpCfg& cfg,
                                            ArpEntry& e) {
  const uint4 r = rec[i];  // lnx_rx_delivery: ip_end; handler | l4_off << 16; the ports; verdict | flags << 8
  const uint32_t handler = r.y & 0xFFFFu;
  if ((r.w & 0xFFu) != 0 || handler < LNX_H_ETH || handler > LNX_H_ETH + 8u) return kArpNone;
  const uint64_t s = off[i];
  const uint32_t L = lnx::frame_len(s, off[i + 1], trim);
  const uint8_t* p = bytes + s;
  if (!arp_reaches(L, 0u, handler, [p](uint32_t o) -> uint32_t { return (lnx::own_byte(p + o) << 8) | lnx::own_byte(p + o + 1u); }))
    return kArpNone;
  if (L < kArpMinL) return kArpNone;  // rule 1, before the body's loads
  const ArBody b = ar_body(p);
  auto byt = [&b](uint32_t o) -> uint32_t { return (b.w[(o - kArpBody) >> 2] >> (8u * ((o - kArpBody) & 3u))) & 0xFFu; };
  uint32_t verdict;
  const uint32_t kind = arp_demux(L, cfg, byt, verdict);
  e = arp_entry_of(byt);
  return kind;
}

// ------------------------------------------------------------------ count, scan
// ws: cnt1[G], then cnt2[G].  The count launch writes entry g of both; the scan
// turns them into the sums before workgroup g.
__global__ void __launch_bounds__(kArBlock)
arp_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint4* __restrict__ rec, ArpCfg cfg, uint32_t* __restrict__ counts) {
  __shared__ uint32_t w1[kArWaves], w2[kArWaves];
  uint64_t lo, hi;
  lnx::slice_bounds(n, kArBlock, lo, hi);
  uint32_t c1 = 0, c2 = 0;
  for (uint64_t c0 = lo; c0 < hi; c0 += kArBlock) {  // (uniform)
    const uint64_t i = c0 + threadIdx.x;
    ArpEntry e;
    const uint32_t kind = i < hi ? ar_kind(bytes, off, trim, rec, i, cfg, e) : kArpNone;
    c1 += kind == kArpRequest ? 1u : 0u;
    c2 += kind == kArpReply ? 1u : 0u;
  }
  c1 = lnx::wave_add(c1);
  c2 = lnx::wave_add(c2);
  if ((threadIdx.x & 63u) == 0) w1[threadIdx.x >> 6] = c1, w2[threadIdx.x >> 6] = c2;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t w = 0; w < kArWaves; ++w) s1 += w1[w], s2 += w2[w];
    counts[blockIdx.x] = s1;
    counts[gridDim.x + blockIdx.x] = s2;
  }
}

// d_n = {replies written, replies wanted, seen written, seen wanted}
__global__ void __launch_bounds__(kArGridCap)
arp_scan_kernel(uint32_t* __restrict__ counts, uint32_t G, uint64_t cap, uint64_t cap_seen, uint32_t* __restrict__ d_n) {
  __shared__ uint32_t part1[kArGridCap], part2[kArGridCap];
  const uint32_t t = threadIdx.x;
  const uint32_t c1 = t < G ? counts[t] : 0u, c2 = t < G ? counts[G + t] : 0u;
  lnx::ScanSlot<uint32_t> s1{part1, c1, 0u}, s2{part2, c2, 0u};
  lnx::block_scan_inclusive<kArGridCap>(s1, s2);  // the two sums in the same rounds
  if (t < G) counts[t] = s1.v - c1, counts[G + t] = s2.v - c2;
  if (t == G - 1u) {  // the last workgroup's inclusive sums: the totals (n < 2^32)
    d_n[0] = s1.v < cap ? s1.v : (uint32_t)cap;
    d_n[1] = s1.v;
    d_n[2] = s2.v < cap_seen ? s2.v : (uint32_t)cap_seen;
    d_n[3] = s2.v;
  }
}

// ------------------------------------------------------------------ the row stage
// A chunk's entries in LDS, by rank: the entry's three dwords, the op in the upper half of the second.
struct ArStage {
  uint32_t d0[kArBlock], d1[kArBlock], d2[kArBlock];
};

// Replies k0 .. k0 + m - 1 from the staged entries 0 .. m - 1: row `row` takes
// entries row, row + 16, ...; lane p of the row makes dword p (arp_plan.hpp
// arp_word), the row XORs the fifteen shares of the FCS and lane 15 holds its
// complement.  The row's sixteen stores are one whole aligned 64-byte block.
// An op other than 1 or 2 (explicit entries only): sixteen zero dwords.
template <bool FCS>
__device__ __forceinline__ void ar_rows(const ArStage& st, const uint32_t* tab, uint32_t m, uint64_t k0, const ArpCfg& cfg,
                                        uint32_t* __restrict__ reply) {
  const uint32_t p = threadIdx.x & 15u, row = threadIdx.x >> 4;
  const uint32_t pw = p < lnx::kRstLanes ? p : lnx::kRstLanes - 1u;
  const uint32_t fixed = arp_fixed_word(pw, cfg);
  for (uint32_t j0 = 0; j0 < m; j0 += kArRows) {  // (uniform: m <= kArBlock, so j < kArBlock; a row past m stores nothing)
    const uint32_t j = j0 + row;
    ArpEntry e;
    e.d0 = st.d0[j], e.d1 = st.d1[j] & 0xFFFFu, e.d2 = st.d2[j];
    const uint32_t op = st.d1[j] >> 16;
    uint32_t w = arp_word(pw, fixed, e, op);
    if (FCS) {
      uint32_t z = lnxr::rst_fcs_part(pw, w, [tab](uint32_t q, uint32_t i, uint32_t v) -> uint32_t { return tab[lnx::rst_nib(q, i, v)]; });
      z = lnx::row_xor16(p < lnx::kRstLanes ? z : 0u);
      w = p < lnx::kRstLanes ? w : ~z;
    } else {
      w = p < lnx::kRstLanes ? w : 0u;
    }
    if (j < m) reply[(k0 + j) * kArpWords + p] = arp_op_ok(op) ? w : 0u;
  }
}

__device__ __forceinline__ void ar_tables(uint32_t* tab, const uint32_t* __restrict__ image) {
  for (uint32_t i = threadIdx.x; i < lnx::kRstImageDwords; i += kArBlock) tab[i] = image[lnx::kRstImgZ + i];
}

// ------------------------------------------------------------------ build
// run1, run2: the frames of kind 1 and of kind 2 before the chunk (the scan's
// bases of this workgroup, then the chunks walked).  A frame's rank in its chunk,
// once per kind: the waves' counts before its wave (through LDS) plus the lanes
// of that kind below it in its wave.  Nothing at or past `cap` (slots, d_src)
// or `cap_seen` (d_seen) is written; seen may be NULL with cap_seen 0.
template <bool FCS>
__global__ void __launch_bounds__(kArBlock)
arp_build_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint4* __restrict__ rec, ArpCfg cfg, uint64_t cap, uint64_t cap_seen,
                 const uint32_t* __restrict__ base, const uint32_t* __restrict__ image, uint32_t* __restrict__ reply,
                 uint32_t* __restrict__ src, uint4* __restrict__ seen) {
  __shared__ uint32_t tab[FCS ? lnx::kRstImageDwords : 1];
  __shared__ ArStage st;
  __shared__ uint32_t wc1[kArWaves], wc2[kArWaves];
  const uint32_t t = threadIdx.x, wave = t >> 6;
  uint64_t run1 = base[blockIdx.x], run2 = base[gridDim.x + blockIdx.x];
  if (run1 >= cap && run2 >= cap_seen) return;  // (uniform) both boundaries lie before this slice
  if (FCS) ar_tables(tab, image);
  uint64_t lo, hi;
  lnx::slice_bounds(n, kArBlock, lo, hi);
  for (uint64_t c0 = lo; c0 < hi && (run1 < cap || run2 < cap_seen); c0 += kArBlock) {  // (uniform: every wave keeps all its lanes)
    const uint64_t i = c0 + t;
    ArpEntry e;
    const uint32_t kind = i < hi ? ar_kind(bytes, off, trim, rec, i, cfg, e) : kArpNone;
    uint32_t below1, n1, below2, n2;
    lnx::wave_rank(kind == kArpRequest, below1, n1);
    lnx::wave_rank(kind == kArpReply, below2, n2);
    __syncthreads();  // the last chunk's rows are done with st and the counts (and, first, the tables' stores)
    if ((t & 63u) == 0) wc1[wave] = n1, wc2[wave] = n2;
    __syncthreads();
    uint32_t before1, total1, before2, total2;
    lnx::waves_before<kArWaves>(wc1, wave, before1, total1);
    lnx::waves_before<kArWaves>(wc2, wave, before2, total2);
    const uint64_t k1 = run1 + before1 + below1, k2 = run2 + before2 + below2;
    if (kind == kArpReply && k2 < cap_seen) seen[k2] = make_uint4(e.d0, e.d1, e.d2, (uint32_t)i);  // lnx_arp_seen
    if (kind == kArpRequest && k1 < cap) {
      const uint32_t r = before1 + below1;  // < kArBlock
      st.d0[r] = e.d0;
      st.d1[r] = e.d1 | (kArpReply << 16);
      st.d2[r] = e.d2;
      src[k1] = (uint32_t)i;
    }
    __syncthreads();
    const uint64_t room = run1 < cap ? cap - run1 : 0u;
    ar_rows<FCS>(st, tab, total1 < room ? total1 : (uint32_t)room, run1, cfg, reply);
    run1 += total1;
    run2 += total2;
  }
}

// ------------------------------------------------------------------ front end: explicit entries
// entry: lnx_arp_entry as three little-endian dwords; reply k from entry k and op k.
template <bool FCS>
__global__ void __launch_bounds__(kArBlock)
arp_frames_kernel(const uint32_t* __restrict__ entry, const uint16_t* __restrict__ op, uint64_t n, ArpCfg cfg,
                  const uint32_t* __restrict__ image, uint32_t* __restrict__ reply) {
  __shared__ uint32_t tab[FCS ? lnx::kRstImageDwords : 1];
  __shared__ ArStage st;
  const uint32_t t = threadIdx.x;
  if (FCS) ar_tables(tab, image);
  for (uint64_t c0 = (uint64_t)blockIdx.x * kArBlock; c0 < n; c0 += (uint64_t)gridDim.x * kArBlock) {  // (uniform)
    const uint64_t i = c0 + t;
    __syncthreads();  // the last chunk's rows are done with st (and, first, the tables' stores)
    if (i < n) {
      const uint32_t* w = entry + 3u * i;
      st.d0[t] = w[0];
      st.d1[t] = (w[1] & 0xFFFFu) | ((uint32_t)op[i] << 16);
      st.d2[t] = w[2];
    }
    __syncthreads();
    const uint64_t left = n - c0;
    ar_rows<FCS>(st, tab, left < (uint64_t)kArBlock ? (uint32_t)left : (uint32_t)kArBlock, c0, cfg, reply);
  }
}

// ------------------------------------------------------------------ launchers
// ws: the workgroups' kind-1 counts, then bases (G words), and the same of kind 2 (G words)
uint64_t arp_ws_bytes(uint64_t n) { return (uint64_t)lnx::slice_grid(n, kArBlock, kArGridCap) * 8u; }

// n > 0.  cap == 0 and cap_seen == 0: d_n alone is written (count and scan).
hipError_t launch_arp_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                            const lnx_rst_cfg& cfg, uint64_t cap, uint64_t cap_seen, uint8_t* reply, uint32_t* src,
                            lnx_arp_seen* seen, uint32_t* d_n, void* ws, const uint32_t* image, hipStream_t stream) {
  const uint32_t G = lnx::slice_grid(n, kArBlock, kArGridCap);
  const ArpCfg c = arp_cfg_of(cfg);
  const uint4* rb = reinterpret_cast<const uint4*>(rec);
  uint32_t* counts = static_cast<uint32_t*>(ws);
  hipError_t e;
  hipLaunchKernelGGL(arp_count_kernel, dim3(G), dim3(kArBlock), 0, stream, bytes, off, n, trim, rb, c, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(arp_scan_kernel, dim3(1), dim3(kArGridCap), 0, stream, counts, G, cap, cap_seen, d_n);
  if ((e = hipGetLastError()) != hipSuccess || (cap == 0 && cap_seen == 0)) return e;
  uint32_t* out = reinterpret_cast<uint32_t*>(reply);
  uint4* sn = reinterpret_cast<uint4*>(seen);
  if (c.fcs)
    hipLaunchKernelGGL(arp_build_kernel<true>, dim3(G), dim3(kArBlock), 0, stream, bytes, off, n, trim, rb, c, cap, cap_seen,
                       counts, image, out, src, sn);
  else
    hipLaunchKernelGGL(arp_build_kernel<false>, dim3(G), dim3(kArBlock), 0, stream, bytes, off, n, trim, rb, c, cap, cap_seen,
                       counts, image, out, src, sn);
  return hipGetLastError();
}

hipError_t launch_arp_frames(const lnx_rst_cfg& cfg, const lnx_arp_entry* entry, const uint16_t* op, uint64_t n, uint8_t* reply,
                             const uint32_t* image, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const ArpCfg c = arp_cfg_of(cfg);
  const uint64_t chunks = (n + kArBlock - 1) / kArBlock;
  const dim3 grid((unsigned)(chunks < kArFramesGridCap ? chunks : kArFramesGridCap));
  const uint32_t* in = reinterpret_cast<const uint32_t*>(entry);
  uint32_t* out = reinterpret_cast<uint32_t*>(reply);
  if (c.fcs)
    hipLaunchKernelGGL(arp_frames_kernel<true>, grid, dim3(kArBlock), 0, stream, in, op, n, c, image, out);
  else
    hipLaunchKernelGGL(arp_frames_kernel<false>, grid, dim3(kArBlock), 0, stream, in, op, n, c, image, out);
  return hipGetLastError();
}

}  // namespace lnxa
