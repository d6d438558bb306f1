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
//          kSlotBlock frames at a time: a thread per frame decides (the front
//          end) and is ranked once per kind by ballot / mbcnt; a kind-2 thread
//          stores its own record; the chunk's kind-1 entries are staged in LDS
//          by rank, and the row stage of slot_frame.hpp writes a reply's 16
//          dwords as one aligned 64-byte block.
// lnx_arp_frames_batch is the row stage behind the other front end: the
// caller's explicit entries and ops (slot_frame.hpp slot_frames).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "arp_plan.hpp"
#include "launch.hpp"
#include "slice_walk.hpp"
#include "slot_frame.hpp"

namespace lnxa {

using lnx::kSlotBlock, lnx::kSlotWaves, lnx::kSlotGridCap;

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
__global__ void __launch_bounds__(kSlotBlock)
arp_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint4* __restrict__ rec, ArpCfg cfg, uint32_t* __restrict__ counts) {
  __shared__ uint32_t w1[kSlotWaves], w2[kSlotWaves];
  uint64_t lo, hi;
  lnx::slice_bounds(n, kSlotBlock, lo, hi);
  uint32_t c1 = 0, c2 = 0;
  for (uint64_t c0 = lo; c0 < hi; c0 += kSlotBlock) {  // (uniform)
    const uint64_t i = c0 + threadIdx.x;
    ArpEntry e;
    const uint32_t kind = i < hi ? ar_kind(bytes, off, trim, rec, i, cfg, e) : kArpNone;
    c1 += kind == kArpRequest ? 1u : 0u;
    c2 += kind == kArpReply ? 1u : 0u;
  }
  lnx::ScanSlot<uint32_t> s1{w1, lnx::wave_add(c1), 0u}, s2{w2, lnx::wave_add(c2), 0u};
  lnx::block_total<kSlotWaves>(s1, s2);
  if (threadIdx.x == 0) counts[blockIdx.x] = s1.v, counts[gridDim.x + blockIdx.x] = s2.v;
}

// d_n = {replies written, replies wanted, seen written, seen wanted}
__global__ void __launch_bounds__(kSlotGridCap)
arp_scan_kernel(uint32_t* __restrict__ counts, uint32_t G, uint64_t cap, uint64_t cap_seen, uint32_t* __restrict__ d_n) {
  __shared__ uint32_t part1[kSlotGridCap], part2[kSlotGridCap];
  const uint32_t t = threadIdx.x;
  const uint32_t c1 = t < G ? counts[t] : 0u, c2 = t < G ? counts[G + t] : 0u;
  lnx::ScanSlot<uint32_t> s1{part1, c1, 0u}, s2{part2, c2, 0u};
  lnx::block_scan_inclusive<kSlotGridCap>(s1, s2);  // the two sums in the same rounds
  if (t < G) counts[t] = s1.v - c1, counts[G + t] = s2.v - c2;
  if (t == G - 1u) {  // the last workgroup's inclusive sums: the totals (n < 2^32)
    lnx::written_wanted(d_n, s1.v, cap);
    lnx::written_wanted(d_n + 2, s2.v, cap_seen);
  }
}

// ------------------------------------------------------------------ the row stage's entries
// A chunk's entries in LDS, by rank: the entry's three dwords, the op in the upper half of the second.
struct ArStage {
  uint32_t d0[kSlotBlock], d1[kSlotBlock], d2[kSlotBlock];
};

// slot_rows' callable: dword pw of staged entry j (arp_plan.hpp arp_word).  An op
// other than 1 or 2 (explicit entries only) clears `live`: sixteen zero dwords.
// The lane's fixed word is made here, once.
__device__ __forceinline__ auto ar_word(const ArStage& st, const ArpCfg& cfg) {
  const uint32_t fixed = arp_fixed_word(lnx::slot_lane_word(), cfg);
  return [&st, fixed](uint32_t pw, uint32_t j, bool& live) -> uint32_t {
    ArpEntry e;
    e.d0 = st.d0[j], e.d1 = st.d1[j] & 0xFFFFu, e.d2 = st.d2[j];
    const uint32_t op = st.d1[j] >> 16;
    live = arp_op_ok(op);
    return arp_word(pw, fixed, e, op);
  };
}

// ------------------------------------------------------------------ build
// run1, run2: the frames of kind 1 and of kind 2 before the chunk (the scan's
// bases of this workgroup, then the chunks walked).  A frame's rank in its chunk,
// once per kind: slice_walk.hpp chunk_rank.  Nothing at or past `cap` (slots, d_src)
// or `cap_seen` (d_seen) is written; seen may be NULL with cap_seen 0.
template <bool FCS>
__global__ void __launch_bounds__(kSlotBlock)
arp_build_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint4* __restrict__ rec, ArpCfg cfg, uint64_t cap, uint64_t cap_seen,
                 const uint32_t* __restrict__ base, const uint32_t* __restrict__ image, uint32_t* __restrict__ reply,
                 uint32_t* __restrict__ src, uint4* __restrict__ seen) {
  __shared__ uint32_t tab[FCS ? lnx::kRstImageDwords : 1];
  __shared__ ArStage st;
  __shared__ uint32_t wc1[kSlotWaves], wc2[kSlotWaves];
  const uint32_t t = threadIdx.x;
  uint64_t run1 = base[blockIdx.x], run2 = base[gridDim.x + blockIdx.x];
  if (run1 >= cap && run2 >= cap_seen) return;  // (uniform) both boundaries lie before this slice
  if (FCS) lnx::slot_tables(tab, image);
  const auto word = ar_word(st, cfg);
  uint64_t lo, hi;
  lnx::slice_bounds(n, kSlotBlock, lo, hi);
  for (uint64_t c0 = lo; c0 < hi && (run1 < cap || run2 < cap_seen); c0 += kSlotBlock) {  // (uniform: every wave keeps all its lanes)
    const uint64_t i = c0 + t;
    ArpEntry e;
    const uint32_t kind = i < hi ? ar_kind(bytes, off, trim, rec, i, cfg, e) : kArpNone;
    lnx::RankSlot q1{wc1, kind == kArpRequest, 0u, 0u}, q2{wc2, kind == kArpReply, 0u, 0u};
    lnx::chunk_rank<kSlotWaves>(q1, q2);  // (its first barrier: the last chunk's rows are done with st, and, first, the tables' stores)
    const uint64_t k1 = run1 + q1.rank, k2 = run2 + q2.rank;
    if (q2.q && k2 < cap_seen) seen[k2] = make_uint4(e.d0, e.d1, e.d2, (uint32_t)i);  // lnx_arp_seen
    if (q1.q && k1 < cap) {
      const uint32_t r = q1.rank;  // < kSlotBlock
      st.d0[r] = e.d0;
      st.d1[r] = e.d1 | (kArpReply << 16);
      st.d2[r] = e.d2;
      src[k1] = (uint32_t)i;
    }
    __syncthreads();
    const uint64_t room = run1 < cap ? cap - run1 : 0u;
    lnx::slot_rows<FCS>(tab, q1.total < room ? q1.total : (uint32_t)room, run1, reply, word);
    run1 += q1.total;
    run2 += q2.total;
  }
}

// ------------------------------------------------------------------ front end: explicit entries
// entry: lnx_arp_entry as three little-endian dwords; reply k from entry k and op k.
struct ArFrames {
  using Stage = ArStage;
  const uint32_t* __restrict__ entry;
  const uint16_t* __restrict__ op;
  const ArpCfg& cfg;
  __device__ __forceinline__ void load(Stage& st, uint32_t t, uint64_t i) const {
    const uint32_t* w = entry + 3u * i;
    st.d0[t] = w[0];
    st.d1[t] = (w[1] & 0xFFFFu) | ((uint32_t)op[i] << 16);
    st.d2[t] = w[2];
  }
  __device__ __forceinline__ auto word(const Stage& st) const { return ar_word(st, cfg); }
};
template <bool FCS>
__global__ void __launch_bounds__(kSlotBlock)
arp_frames_kernel(const uint32_t* __restrict__ entry, const uint16_t* __restrict__ op, uint64_t n, ArpCfg cfg,
                  const uint32_t* __restrict__ image, uint32_t* __restrict__ reply) {
  lnx::slot_frames<FCS>(ArFrames{entry, op, cfg}, n, image, reply);
}

// ------------------------------------------------------------------ launchers
// ws: the workgroups' kind-1 counts, then bases (G words), and the same of kind 2 (G words)
uint64_t arp_ws_bytes(uint64_t n) { return (uint64_t)lnx::slice_grid(n, kSlotBlock, kSlotGridCap) * 8u; }

// n > 0.  cap == 0 and cap_seen == 0: d_n alone is written (count and scan).
hipError_t launch_arp_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                            const lnx_rst_cfg& cfg, uint64_t cap, uint64_t cap_seen, uint8_t* reply, uint32_t* src,
                            lnx_arp_seen* seen, uint32_t* d_n, void* ws, const uint32_t* image, hipStream_t stream) {
  const uint32_t G = lnx::slice_grid(n, kSlotBlock, kSlotGridCap);
  const ArpCfg c = arp_cfg_of(cfg);
  const uint4* rb = reinterpret_cast<const uint4*>(rec);
  uint32_t* counts = static_cast<uint32_t*>(ws);
  hipError_t e;
  hipLaunchKernelGGL(arp_count_kernel, dim3(G), dim3(kSlotBlock), 0, stream, bytes, off, n, trim, rb, c, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(arp_scan_kernel, dim3(1), dim3(kSlotGridCap), 0, stream, counts, G, cap, cap_seen, d_n);
  if ((e = hipGetLastError()) != hipSuccess || (cap == 0 && cap_seen == 0)) return e;
  return lnx::launch_fcs(c.fcs, arp_build_kernel<true>, arp_build_kernel<false>, dim3(G), dim3(kSlotBlock), stream, bytes, off, n,
                         trim, rb, c, cap, cap_seen, counts, image, reinterpret_cast<uint32_t*>(reply), src,
                         reinterpret_cast<uint4*>(seen));
}

hipError_t launch_arp_frames(const lnx_rst_cfg& cfg, const lnx_arp_entry* entry, const uint16_t* op, uint64_t n, uint8_t* reply,
                             const uint32_t* image, hipStream_t stream) {
  const ArpCfg c = arp_cfg_of(cfg);
  return lnx::launch_slot_frames(c.fcs, arp_frames_kernel<true>, arp_frames_kernel<false>, n, stream,
                                 reinterpret_cast<const uint32_t*>(entry), op, n, c, image, reinterpret_cast<uint32_t*>(reply));
}

}  // namespace lnxa
