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
//          kSlotBlock frames at a time: a thread per frame decides and reads the
//          frame's fields (the front end), the chunk's entries are ranked by
//          ballot / mbcnt and staged in LDS, and the row stage of slot_frame.hpp
//          writes a reply's 16 dwords as one aligned 64-byte block.
// lnx_tcp_rst_frames_batch is the row stage behind the other front end: the
// caller's explicit entries (slot_frame.hpp slot_frames).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.hpp"
#include "reply_plan.hpp"
#include "slice_walk.hpp"
#include "slot_frame.hpp"

namespace lnxr {

using lnx::kSlotBlock, lnx::kSlotWaves, lnx::kSlotGridCap;

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
__global__ void __launch_bounds__(kSlotBlock)
rst_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint8_t* __restrict__ rec, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kSlotWaves];
  uint64_t lo, hi;
  lnx::slice_bounds(n, kSlotBlock, lo, hi);
  uint32_t c = 0;
  for (uint64_t c0 = lo; c0 < hi; c0 += kSlotBlock) {  // (uniform)
    const uint64_t i = c0 + threadIdx.x;
    const uint8_t* p = bytes;
    uint32_t l4 = 0;
    if (i < hi && rp_queues(bytes, off, trim, rec, i, p, l4)) c += 1u;
  }
  lnx::ScanSlot<uint32_t> s{wsum, lnx::wave_add(c), 0u};
  lnx::block_total<kSlotWaves>(s);
  if (threadIdx.x == 0) counts[blockIdx.x] = s.v;
}

// counts[g] becomes the queueing frames in the workgroups before g; d_n = {written, wanted}
__global__ void __launch_bounds__(kSlotGridCap)
rst_scan_kernel(uint32_t* __restrict__ counts, uint32_t G, uint64_t cap, uint32_t* __restrict__ d_n) {
  __shared__ uint32_t part[kSlotGridCap];
  const uint32_t t = threadIdx.x;
  const uint32_t c = t < G ? counts[t] : 0u;
  const uint32_t inc = lnx::block_scan_inclusive<kSlotGridCap>(part, c);
  if (t < G) counts[t] = inc - c;
  if (t == G - 1u) lnx::written_wanted(d_n, inc, cap);  // the last workgroup's inclusive sum: the total (n < 2^32)
}

// ------------------------------------------------------------------ the row stage's entries
// A chunk's entries in LDS, by rank: the address, remote | local << 16, seq, ack, flags | IP ID << 16.
struct RpStage {
  uint32_t addr[kSlotBlock], ports[kSlotBlock], seq[kSlotBlock], ack[kSlotBlock], flid[kSlotBlock];
};

// slot_rows' callable: dword pw of staged entry j (reply_plan.hpp rst_word; every
// lane takes the two sums, a handful of adds).  The lane's fixed word is made here, once.
__device__ __forceinline__ auto rp_word(const RpStage& st, const RstCfg& cfg) {
  const uint32_t fixed = rst_fixed_word(lnx::slot_lane_word(), cfg);
  return [&st, &cfg, fixed](uint32_t pw, uint32_t j, bool&) -> uint32_t {
    RstEntry e;
    e.addr = st.addr[j];
    e.remote_port = st.ports[j] & 0xFFFFu, e.local_port = st.ports[j] >> 16;
    e.seq = st.seq[j], e.ack = st.ack[j];
    e.flags = st.flid[j] & 0xFFFFu;
    const uint32_t id = st.flid[j] >> 16;
    return rst_word(pw, fixed, e, id, rst_ip_sum(cfg, e, id), rst_tcp_sum(cfg, e));
  };
}

// ------------------------------------------------------------------ build
// run: the queueing frames before the chunk (the scan's base of this workgroup,
// then the chunks walked).  A frame's rank in its chunk: slice_walk.hpp chunk_rank.
// Nothing at or past `cap` is written: no slot, no d_src entry, and no ID is read.
template <bool FCS>
__global__ void __launch_bounds__(kSlotBlock)
rst_reply_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                 const uint8_t* __restrict__ rec, RstCfg cfg, const uint16_t* __restrict__ ip_id, uint64_t cap,
                 const uint32_t* __restrict__ base, const uint32_t* __restrict__ image, uint32_t* __restrict__ reply,
                 uint32_t* __restrict__ src) {
  __shared__ uint32_t tab[FCS ? lnx::kRstImageDwords : 1];
  __shared__ RpStage st;
  __shared__ uint32_t wcnt[kSlotWaves];
  const uint32_t t = threadIdx.x;
  if (FCS) lnx::slot_tables(tab, image);
  const auto word = rp_word(st, cfg);
  uint64_t lo, hi;
  lnx::slice_bounds(n, kSlotBlock, lo, hi);
  uint64_t run = base[blockIdx.x];
  for (uint64_t c0 = lo; c0 < hi && run < cap; c0 += kSlotBlock) {  // (uniform: every wave keeps all its lanes)
    const uint64_t i = c0 + t;
    const uint8_t* p = bytes;
    uint32_t l4 = 0;
    lnx::RankSlot k{wcnt, i < hi && rp_queues(bytes, off, trim, rec, i, p, l4), 0u, 0u};
    lnx::chunk_rank<kSlotWaves>(k);  // (its first barrier: the last chunk's rows are done with st, and, first, the tables' stores)
    const uint32_t r = k.rank;  // < kSlotBlock
    if (k.q && run + r < cap) {
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
    lnx::slot_rows<FCS>(tab, k.total < room ? k.total : (uint32_t)room, run, reply, word);
    run += k.total;
  }
}

// ------------------------------------------------------------------ front end: explicit entries
// entry: lnx_tcp_rst as five little-endian dwords (the address bytes, remote |
// local << 16, seq, ack, flags | zero << 16); reply k from entry k.
struct RpFrames {
  using Stage = RpStage;
  const uint32_t* __restrict__ entry;
  const uint16_t* __restrict__ ip_id;
  const RstCfg& cfg;
  __device__ __forceinline__ void load(Stage& st, uint32_t t, uint64_t i) const {
    const uint32_t* w = entry + 5u * i;
    st.addr[t] = __builtin_bswap32(w[0]);
    st.ports[t] = w[1];
    st.seq[t] = w[2];
    st.ack[t] = w[3];
    st.flid[t] = (w[4] & 0xFFFFu) | ((uint32_t)ip_id[i] << 16);
  }
  __device__ __forceinline__ auto word(const Stage& st) const { return rp_word(st, cfg); }
};
template <bool FCS>
__global__ void __launch_bounds__(kSlotBlock)
rst_frames_kernel(const uint32_t* __restrict__ entry, uint64_t n, RstCfg cfg, const uint16_t* __restrict__ ip_id,
                  const uint32_t* __restrict__ image, uint32_t* __restrict__ reply) {
  lnx::slot_frames<FCS>(RpFrames{entry, ip_id, cfg}, n, image, reply);
}

// ------------------------------------------------------------------ launchers
// ws: the workgroups' counts, then bases (G words)
uint64_t rst_ws_bytes(uint64_t n) { return (uint64_t)lnx::slice_grid(n, kSlotBlock, kSlotGridCap) * 4u; }

// n > 0.  cap == 0: d_n alone is written (count and scan).
hipError_t launch_rst_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                            const lnx_rst_cfg& cfg, const uint16_t* ip_id, uint64_t cap, uint8_t* reply, uint32_t* src,
                            uint32_t* d_n, void* ws, const uint32_t* image, hipStream_t stream) {
  const uint32_t G = lnx::slice_grid(n, kSlotBlock, kSlotGridCap);
  const RstCfg c = rst_cfg_of(cfg);
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(rec);
  uint32_t* counts = static_cast<uint32_t*>(ws);
  hipError_t e;
  hipLaunchKernelGGL(rst_count_kernel, dim3(G), dim3(kSlotBlock), 0, stream, bytes, off, n, trim, rb, counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(rst_scan_kernel, dim3(1), dim3(kSlotGridCap), 0, stream, counts, G, cap, d_n);
  if ((e = hipGetLastError()) != hipSuccess || cap == 0) return e;
  return lnx::launch_fcs(c.fcs, rst_reply_kernel<true>, rst_reply_kernel<false>, dim3(G), dim3(kSlotBlock), stream, bytes, off, n,
                         trim, rb, c, ip_id, cap, counts, image, reinterpret_cast<uint32_t*>(reply), src);
}

hipError_t launch_rst_frames(const lnx_rst_cfg& cfg, const lnx_tcp_rst* entry, uint64_t n, const uint16_t* ip_id,
                             uint8_t* reply, const uint32_t* image, hipStream_t stream) {
  const RstCfg c = rst_cfg_of(cfg);
  return lnx::launch_slot_frames(c.fcs, rst_frames_kernel<true>, rst_frames_kernel<false>, n, stream,
                                 reinterpret_cast<const uint32_t*>(entry), n, c, ip_id, image, reinterpret_cast<uint32_t*>(reply));
}

}  // namespace lnxr
