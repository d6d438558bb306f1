// echo_kernel.hip — echo replies for ICMPv4 echo requests on gfx950 (DESIGN.md
// §3.20): the frame of every delivery record that queues an echo entry
// (echo_plan.hpp), in arrival order, each in whole 64-byte blocks of d_reply.
//
// Three launches on the caller's stream, the slice walk of slice_walk.hpp, none
// of which waits for another workgroup (no look-back, no grid barrier, no spin,
// no global atomics; the launches' order on the stream is the only dependency):
//   count  each workgroup counts the queueing frames of ONE contiguous index
//          slice and the blocks their replies take (from the records and the
//          few header bytes of rules 3-4; the data is never read);
//   scan   over the workgroups in index order (one workgroup): two running
//          sums, replies and blocks, and d_n;
//   build  each workgroup walks its slice again in index order, a chunk of
//          kEpBlock frames at a time: a thread per frame decides, ranks its
//          reply and its first block (ballot / mbcnt, a wave prefix sum) and
//          stages the entry in LDS; then a 16-lane row per reply of one or two
//          blocks and a wave per longer reply stream the request's data from
//          its own aligned dwords, realign it to the reply's phase, take the
//          ICMP checksum over the reply's own dwords and write whole aligned
//          64-byte blocks, the FCS folded over the same dwords (a row joins its
//          lanes' shares every step; a wave's lanes each keep a register of
//          their own and are joined once a reply).
// The checksum stands in the header, which the FCS covers, so a reply's data is
// needed twice: a row keeps its two dwords a lane in registers, a wave up to
// eight (2048 bytes, any MTU-sized reply: the loads of the whole reply are in
// flight together), and only a longer reply is read twice by its wave (the
// second read comes from the cache).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "echo_plan.hpp"
#include "launch.hpp"
#include "slice_walk.hpp"
#include "slot_frame.hpp"
#include "table_layout.hpp"

namespace lnxe {

// (kEpBlock, kEpGridCap, kEpRowBlocks and kEpWaveBlocks are restated in tests/test_echo_reply_gpu.py)
constexpr int kEpBlock = 256;                  // frames per chunk: one per thread (tests: CHUNK)
constexpr uint32_t kEpWaves = kEpBlock / 64, kEpRows = kEpBlock / 16;
constexpr uint32_t kEpGridCap = 1024;          // workgroups of the count / build launches (tests: GRID_CAP)
constexpr uint32_t kEpRowBlocks = 2;           // a reply of at most this many blocks takes a row, a longer one a wave (tests: ROW_BLOCKS)
constexpr uint32_t kEpRowSteps = kEpRowBlocks; // 16 dwords a step
// a wave keeps a reply of up to kEpWaveSteps 64-dword steps (2048 bytes: any MTU-sized one) in registers, its loads in
// flight together; a longer one is read twice (tests: WAVE_BLOCKS)
constexpr uint32_t kEpWaveSteps = 8, kEpWaveBlocks = 4 * kEpWaveSteps;

// Frame i under record i: does it queue an entry (rules 1-4)?  A frame whose
// record has another handler or verdict costs its record and nothing else; a
// candidate its two offsets and bytes l4 and 14.  p, l4, end: the frame's start
// and the record's l4_off and ip_end, for the build.
__device__ __forceinline__ bool ep_queues(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                          uint32_t trim, const uint4* __restrict__ rec, uint64_t i, const uint8_t*& p,
                                          uint32_t& l4, uint32_t& end) {
  const uint4 r = rec[i];  // lnx_rx_delivery: ip_end; handler | l4_off << 16; the ports; verdict | flags << 8
  if ((r.w & 0xFFu) != 0 || (r.y & 0xFFFFu) != kHandlerIcmp4) return false;
  const uint64_t s = off[i];
  const uint32_t L = lnx::frame_len(s, off[i + 1], trim);
  p = bytes + s;
  l4 = r.y >> 16;
  end = r.x;
  const uint8_t* pp = p;
  return echo_queues(L, 0u, kHandlerIcmp4, l4, end, [pp](uint32_t o) -> uint32_t { return lnx::own_byte(pp + o); });
}

// ------------------------------------------------------------------ count, scan
// ws: blk[G + 1] (uint64), then cnt[G + 1] (uint32).  The count launch writes entry g
// of both; the scan turns them into the sums before workgroup g, entry G the totals.
// a block count as d_n reports it: saturating at 2^32 - 1
__device__ __forceinline__ uint32_t ep_sat32(uint64_t v) { return v < 0xFFFFFFFFull ? (uint32_t)v : 0xFFFFFFFFu; }
__device__ __forceinline__ uint64_t* ep_ws_blk(void* ws) { return static_cast<uint64_t*>(ws); }
__device__ __forceinline__ uint32_t* ep_ws_cnt(void* ws, uint32_t G) { return reinterpret_cast<uint32_t*>(static_cast<uint64_t*>(ws) + G + 1u); }

__global__ void __launch_bounds__(kEpBlock)
echo_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                  const uint4* __restrict__ rec, uint32_t fcs, void* __restrict__ ws) {
  __shared__ uint32_t wcnt[kEpWaves];
  __shared__ uint64_t wblk[kEpWaves];
  uint64_t lo, hi;
  lnx::slice_bounds(n, kEpBlock, lo, hi);
  uint32_t c = 0;
  uint64_t b = 0;
  for (uint64_t c0 = lo; c0 < hi; c0 += kEpBlock) {  // (uniform)
    const uint64_t i = c0 + threadIdx.x;
    const uint8_t* p = bytes;
    uint32_t l4 = 0, end = 0;
    const bool q = i < hi && ep_queues(bytes, off, trim, rec, i, p, l4, end);
    c += lnx::wave_add(q ? 1u : 0u);
    b += lnx::wave_add(q ? echo_blocks(end - l4 - 8u, fcs) : 0u);  // (a chunk's blocks fit 32 bits)
  }
  lnx::ScanSlot<uint32_t> sc{wcnt, c, 0u};
  lnx::ScanSlot<uint64_t> sb{wblk, b, 0u};
  lnx::block_total<kEpWaves>(sc, sb);
  if (threadIdx.x == 0) ep_ws_cnt(ws, gridDim.x)[blockIdx.x] = sc.v, ep_ws_blk(ws)[blockIdx.x] = sb.v;
}

// d_n = {written, wanted, blocks written, blocks wanted}.  When the totals exceed a
// capacity, written and blocks written are 0 here and the build launch's boundary
// workgroup writes them (echo_reply_kernel).
__global__ void __launch_bounds__(kEpGridCap)
echo_scan_kernel(void* __restrict__ ws, uint32_t G, uint64_t cap, uint64_t cap_blocks, uint32_t* __restrict__ d_n) {
  __shared__ uint32_t part[kEpGridCap];
  __shared__ uint64_t partb[kEpGridCap];
  uint32_t* cnt = ep_ws_cnt(ws, G);
  uint64_t* blk = ep_ws_blk(ws);
  const uint32_t t = threadIdx.x;
  const uint32_t c = t < G ? cnt[t] : 0u;
  const uint64_t b = t < G ? blk[t] : 0u;
  lnx::ScanSlot<uint32_t> sc{part, c, 0u};
  lnx::ScanSlot<uint64_t> sb{partb, b, 0u};
  lnx::block_scan_inclusive<kEpGridCap>(sc, sb);  // the two sums in the same rounds
  if (t < G) cnt[t] = sc.v - c, blk[t] = sb.v - b;
  if (t == G - 1u) {  // the last workgroup's inclusive sums: the totals
    const uint32_t total = sc.v;  // (n < 2^32)
    const uint64_t totalb = sb.v;
    cnt[G] = total, blk[G] = totalb;
    const bool fits = total <= cap && totalb <= cap_blocks;
    d_n[0] = fits ? total : 0u;
    d_n[1] = total;
    d_n[2] = fits ? ep_sat32(totalb) : 0u;
    d_n[3] = ep_sat32(totalb);
  }
}

// ------------------------------------------------------------------ the copy stage
// A chunk's written entries in LDS, by rank: the request's start, its l4_off and
// ip_end, the remote address, id, the IP ID, the reply's first block (relative to
// the chunk's) and its blocks.
struct EpStage {
  uint32_t plo[kEpBlock], phi[kEpBlock], l4[kEpBlock], end[kEpBlock], addr[kEpBlock], ids[kEpBlock], blk[kEpBlock], nb[kEpBlock];
};

// The XOR / sum over a group of W lanes, in every lane of it: a row, or the wave
// (every lane of the wave is active there).
template <uint32_t W>
__device__ __forceinline__ uint32_t ep_group_xor(uint32_t v) {
  v = lnx::row_xor16(v);
  if (W == 64)
    v = (uint32_t)__builtin_amdgcn_readlane((int)v, 0) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 16) ^
        (uint32_t)__builtin_amdgcn_readlane((int)v, 32) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return v;
}
template <uint32_t W>
__device__ __forceinline__ uint32_t ep_group_add(uint32_t v) {
  return W == 64 ? lnx::wave_add(v) : lnx::row_add16(v);
}

// Dword q >= 10 of the reply.  From byte 38 on the reply is the request from
// l4 + 4 on (id, seq, the data), so with c = the request's byte that lands on
// reply byte 0 (start + l4 - 34) it is the four bytes at c + 4q, those below E
// (= start + ip_end) kept and zero past them: the padding.  Two aligned loads at
// any byte phase, each of a dword that holds a byte of the request below E.  The
// loads are unconditional, so that a reply's loads issue back to back: one that
// has no such dword to fetch takes the dword of reply byte 40 instead (the
// request's seq, l4 + 6 < ip_end: always the request's own), and its value is
// masked away.
__device__ __forceinline__ uint32_t ep_data_word(const uint8_t* c, const uint8_t* E, uint32_t q) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(c) + 4u * (uintptr_t)q, e = reinterpret_cast<uintptr_t>(E);
  const uintptr_t safe = (reinterpret_cast<uintptr_t>(c) + 40u) & ~(uintptr_t)3;
  const uintptr_t al = a & ~(uintptr_t)3;
  const uint32_t sh = 8u * (uint32_t)(a & 3u);
  const uint32_t lo = *reinterpret_cast<const uint32_t*>(a < e ? al : safe);
  const uint32_t hi = *reinterpret_cast<const uint32_t*>(al + 4 < e ? al + 4 : safe);
  const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
  const uint64_t left = a < e ? e - a : 0u;
  return left >= 4 ? v : v & ~lnx::keep_from((int32_t)left);
}

// One reply by a group of W lanes (lane: 0 .. W - 1), entry j of the stage; `act`
// false (rows only): the group goes through the motions, its loads all take the
// staged entry's dword of reply byte 40, and it stores nothing.  STEPS: the steps of W dwords, 0 for as many as the reply has (W = 64:
// the whole wave works on one entry, so the trip count is wave-uniform).
template <uint32_t W, uint32_t STEPS, bool FCS>
__device__ __forceinline__ void ep_reply(const EpStage& st, uint32_t j, bool act, uint32_t lane, uint32_t fixed,
                                         const uint32_t* tab, const RstCfg& cfg, uint64_t blk0, uint32_t* __restrict__ reply) {
  const uint32_t l4 = st.l4[j], end = act ? st.end[j] : l4 + 8u;
  const uint8_t* p = reinterpret_cast<const uint8_t*>(((uint64_t)st.phi[j] << 32) | st.plo[j]);
  const uint8_t* c = p + l4 - kEchoMinL4;
  const uint8_t* E = act ? p + end : c;          // (an idle group: every dword lies at or past E)
  const uint32_t d = end - l4 - 8u;
  const uint32_t nb = act ? st.nb[j] : 0u, ndw = nb * 16u;
  const uint32_t padded = echo_padded(d), nfull = padded >> 2, rem = padded & 3u;
  const uint32_t addr = st.addr[j], id = st.ids[j] & 0xFFFFu, ip_id = st.ids[j] >> 16;
  uint32_t* out = reply + (blk0 + st.blk[j]) * 16u;
  const uint32_t steps = STEPS ? STEPS : (ndw + W - 1u) / W;
  // (W = 64, kept: the steps past the reply's blocks are skipped, wave-uniformly)
  const uint32_t live = W == 64 && STEPS ? (uint32_t)__builtin_amdgcn_readfirstlane((int)((ndw + W - 1u) / W)) : steps;

  // the ICMP checksum: id (the upper half of dword 9, as it lies in memory), then dwords 10 .. of the reply
  uint32_t kept[STEPS ? STEPS : 1];
  uint32_t acc = lane == 0 ? (((id & 0xFFu) << 8) | (id >> 8)) : 0u;
  if (STEPS) {
#pragma unroll
    for (uint32_t s = 0; s < (STEPS ? STEPS : 1); ++s) {
      const uint32_t q = s * W + lane;
      const uint32_t w = ep_data_word(c, E, q >= kEchoHdrWords ? q : kEchoHdrWords);  // (no branch: the loads of all the steps issue together)
      kept[s] = q >= kEchoHdrWords ? w : 0u;
    }
#pragma unroll
    for (uint32_t s = 0; s < (STEPS ? STEPS : 1); ++s) acc = lnx::dot2(kept[s], acc);
  } else {
    for (uint32_t s = 0; s < steps; ++s) {  // (wave-uniform)
      const uint32_t q = s * W + lane;
      acc = lnx::dot2(q >= kEchoHdrWords ? ep_data_word(c, E, q) : 0u, acc);
    }
  }
  const uint32_t icmp_sum = echo_icmp_sum_le(ep_group_add<W>(acc));
  const uint32_t ip_sum = echo_ip_sum(cfg, addr, d, ip_id);
  const uint32_t head = echo_word(lane < kEchoHdrWords ? lane : kEchoHdrWords - 1u, fixed, addr, id, d, ip_id, ip_sum, icmp_sum);

  // the copy, and the FCS over the nfull whole dwords below `padded`: in step s lane p holds dword
  // s W + p.  A row: m of the step's dwords count, and the register before them is folded into the first.
  uint32_t reg = 0xFFFFFFFFu, own = 0u;
  const uint32_t sfull = W == 64 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(nfull / W)) : 0u;
  const uint32_t mlast = W == 64 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(nfull % W)) : 0u;
  for (uint32_t s = 0; s < steps; ++s) {  // (STEPS: a constant; else wave-uniform)
    if (STEPS && s >= live) break;
    const uint32_t q = s * W + lane;
    uint32_t w;
    if (STEPS)
      w = kept[STEPS ? s : 0];
    else
      w = q >= kEchoHdrWords ? ep_data_word(c, E, q) : 0u;
    if (q < kEchoHdrWords) w = head;
    if (FCS) {
      auto at = [tab](uint32_t tt, uint32_t i, uint32_t v) -> uint32_t { return tab[lnx::echo_nib(tt, i, v)]; };
      if (W == 64) {
        // whole steps: the lane's own register (echo_plan.hpp echo_fcs_step), no exchange; the step that
        // holds the last m whole dwords: the lanes' registers joined, then as a row does it
        if (s < sfull) {
          const uint32_t a = echo_fcs_step(own, [tab](uint32_t k, uint32_t e) -> uint32_t { return tab[lnx::byte4_at(lnx::kEchoImgB, k, e)]; });
          own = a ^ w ^ (s == 0 && lane == 0 ? 0xFFFFFFFFu : 0u);
        } else if (s == sfull) {
          if (sfull != 0) reg = ep_group_xor<W>(echo_fcs_part(W - lane, own, at));
          if (mlast != 0) reg = ep_group_xor<W>(lane < mlast ? echo_fcs_part(mlast - lane, lane == 0 ? w ^ reg : w, at) : 0u);
        }
      } else {
        const uint32_t base = s * W;
        const uint32_t m = nfull > base ? (nfull - base < W ? nfull - base : W) : 0u;
        const uint32_t z = ep_group_xor<W>(lane < m ? echo_fcs_part(m - lane, lane == 0 ? w ^ reg : w, at) : 0u);
        reg = m ? z : reg;
      }
      // dword nfull (and the next, when the FCS straddles two) is stored below, with the FCS in it
      if (q < ndw && q != nfull && !(rem != 0 && q == nfull + 1u)) out[q] = w;
    } else {
      if (q < ndw) out[q] = w;
    }
  }
  if (FCS) {
    // nfull >= 15: a data dword, or padding
    const uint32_t last = ep_data_word(c, E, nfull);  // (every lane the same dword; zero at and past `padded`)
    for (uint32_t k = 0; k < rem; ++k) reg = echo_crc_byte(reg, last >> (8u * k));
    const uint32_t fcs = ~reg;
    if (act && lane == 0) out[nfull] = last | (fcs << (8u * rem));
    if (act && lane == 1 && rem != 0) out[nfull + 1u] = fcs >> (32u - 8u * rem);
  }
}

__device__ __forceinline__ void ep_tables(uint32_t* tab, const uint32_t* __restrict__ image) {
  for (uint32_t i = threadIdx.x; i < lnx::kEchoImageDwords; i += kEpBlock) tab[i] = image[lnx::kEchoImgZ + i];
}

// ------------------------------------------------------------------ build
// run, brun: the queueing frames and their blocks before the chunk (the scan's
// bases of this workgroup, then the chunks walked).  Reply k with first block b
// and nb blocks is written iff k < cap and b + nb <= cap_blocks: both sums are
// monotone, so the written replies are a prefix, of the batch and of every
// chunk.  The boundary workgroup, the one whose first reply would fit and whose
// last does not, writes d_n[0] and d_n[2] (the scan wrote them when every reply
// fits).  Nothing at or past the boundary is written and no ID there is read.
template <bool FCS>
__global__ void __launch_bounds__(kEpBlock)
echo_reply_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                  const uint4* __restrict__ rec, RstCfg cfg, const uint16_t* __restrict__ ip_id, uint64_t cap,
                  uint64_t cap_blocks, void* __restrict__ ws, const uint32_t* __restrict__ image,
                  uint32_t* __restrict__ reply, uint64_t* __restrict__ start, uint32_t* __restrict__ len,
                  uint32_t* __restrict__ src, uint32_t* __restrict__ d_n) {
  __shared__ uint32_t tab[FCS ? lnx::kEchoImageDwords : 1];
  __shared__ EpStage st;
  __shared__ uint32_t wcnt[kEpWaves], wblk[kEpWaves], wwr[kEpWaves], wshort[kEpWaves];
  const uint32_t t = threadIdx.x, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
  const uint32_t G = gridDim.x;
  uint64_t run = ep_ws_cnt(ws, G)[blockIdx.x], brun = ep_ws_blk(ws)[blockIdx.x];
  const uint64_t run_end = ep_ws_cnt(ws, G)[blockIdx.x + 1u], brun_end = ep_ws_blk(ws)[blockIdx.x + 1u];
  if (run > cap || brun > cap_blocks) return;  // (uniform) the boundary lies before this slice
  const bool boundary = run_end > cap || brun_end > cap_blocks;  // else all of the slice is written
  if (run == cap || brun == cap_blocks) {  // (uniform) no room left: nothing of this slice is written
    if (boundary && t == 0) d_n[0] = (uint32_t)run, d_n[2] = ep_sat32(brun);
    return;
  }
  if (FCS) ep_tables(tab, image);
  const uint32_t fixed16 = echo_fixed_word((t & 15u) < kEchoHdrWords ? (t & 15u) : kEchoHdrWords - 1u, cfg);
  const uint32_t fixed64 = echo_fixed_word((t & 63u) < kEchoHdrWords ? (t & 63u) : kEchoHdrWords - 1u, cfg);
  uint64_t lo, hi;
  lnx::slice_bounds(n, kEpBlock, lo, hi);
  for (uint64_t c0 = lo; c0 < hi && run < cap && brun < cap_blocks; c0 += kEpBlock) {  // (uniform: every wave keeps all its lanes)
    const uint64_t i = c0 + t;
    const uint8_t* p = bytes;
    uint32_t l4 = 0, end = 0;
    const bool q = i < hi && ep_queues(bytes, off, trim, rec, i, p, l4, end);
    const uint32_t d = q ? end - l4 - 8u : 0u;
    const uint32_t nb = q ? echo_blocks(d, FCS) : 0u;
    uint32_t below, wq;
    lnx::wave_rank(q, below, wq);
    const uint32_t binc = lnx::wave_scan_add(nb);
    __syncthreads();  // the last chunk's rows and waves are done with st and the counts (and, first, the tables' stores)
    if ((t & 63u) == 0) wcnt[wave] = wq;
    if ((t & 63u) == 63u) wblk[wave] = binc;
    __syncthreads();
    uint32_t before, total, bbefore, btotal;
    lnx::waves_before<kEpWaves>(wcnt, wave, before, total);
    lnx::waves_before<kEpWaves>(wblk, wave, bbefore, btotal);
    const uint32_t r = before + below;           // < kEpBlock
    const uint32_t b = bbefore + binc - nb;      // the reply's first block, from the chunk's
    const bool wr = q && run + r < cap && brun + b + nb <= cap_blocks;
    const uint64_t w64 = __builtin_amdgcn_ballot_w64(wr);
    const uint64_t s64 = __builtin_amdgcn_ballot_w64(wr && nb <= kEpRowBlocks);
    if ((t & 63u) == 0) wwr[wave] = (uint32_t)__builtin_popcountll(w64), wshort[wave] = (uint32_t)__builtin_popcountll(s64);
    if (wr) {
      const uint8_t* pp = p;
      const uint32_t id = (lnx::own_byte(pp + l4 + 4u) << 8) | lnx::own_byte(pp + l4 + 5u);
      uint32_t addr = 0;
      for (uint32_t k = 0; k < 4; ++k) addr = (addr << 8) | lnx::own_byte(pp + 26u + k);
      st.plo[r] = (uint32_t)reinterpret_cast<uintptr_t>(p);
      st.phi[r] = (uint32_t)(reinterpret_cast<uintptr_t>(p) >> 32);
      st.l4[r] = l4;
      st.end[r] = end;
      st.addr[r] = addr;
      st.ids[r] = id | ((uint32_t)ip_id[run + r] << 16);
      st.blk[r] = b;
      st.nb[r] = nb;
      start[run + r] = (brun + b) * 64u;
      len[run + r] = echo_len(d, FCS);
      src[run + r] = (uint32_t)i;
    }
    __syncthreads();
    uint32_t m = 0, nshort = 0;
#pragma unroll
    for (uint32_t w = 0; w < kEpWaves; ++w) m += wwr[w], nshort += wshort[w];
    // the written entries are ranks 0 .. m - 1.  Rows: entry row, row + 16, ... when it is short
    if (nshort != 0) {
      const uint32_t lane = t & 15u, row = t >> 4;
      for (uint32_t j0 = 0; j0 < m; j0 += kEpRows) {  // (uniform; an idle row stores nothing)
        const uint32_t j = j0 + row;
        const bool act = j < m && st.nb[j < m ? j : 0u] <= kEpRowBlocks;
        ep_reply<16, kEpRowSteps, FCS>(st, j < m ? j : 0u, act, lane, fixed16, tab, cfg, brun, reply);
      }
    }
    // waves: entry wave, wave + 4, ... when it is long
    if (nshort != m) {
      for (uint32_t j = wave; j < m; j += kEpWaves) {  // (wave-uniform)
        const uint32_t nbj = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.nb[j]);
        if (nbj > kEpWaveBlocks)
          ep_reply<64, 0, FCS>(st, j, true, t & 63u, fixed64, tab, cfg, brun, reply);
        else if (nbj > kEpRowBlocks)
          ep_reply<64, kEpWaveSteps, FCS>(st, j, true, t & 63u, fixed64, tab, cfg, brun, reply);
      }
    }
    if (boundary && m != total) {  // (uniform) the boundary lies in this chunk: its first m replies are the batch's last
      if (t == 0) {
        d_n[0] = (uint32_t)(run + m);
        d_n[2] = ep_sat32(brun + (m ? st.blk[m - 1u] + st.nb[m - 1u] : 0u));
      }
      return;
    }
    run += total;
    brun += btotal;
  }
  // the boundary fell between two chunks (or behind the last one walked)
  if (boundary && t == 0) d_n[0] = (uint32_t)run, d_n[2] = ep_sat32(brun);
}

// ------------------------------------------------------------------ launchers
// ws: the workgroups' block sums (G + 1 qwords), then their reply counts (G + 1 words)
uint64_t echo_ws_bytes(uint64_t n) { return (uint64_t)(lnx::slice_grid(n, kEpBlock, kEpGridCap) + 1u) * 12u; }

// n > 0.  cap == 0 or cap_blocks == 0: d_n alone is written (count and scan).
hipError_t launch_echo_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                             const lnx_rst_cfg& cfg, const uint16_t* ip_id, uint64_t cap, uint64_t cap_blocks, uint8_t* reply,
                             uint64_t* start, uint32_t* len, uint32_t* src, uint32_t* d_n, void* ws, const uint32_t* image,
                             hipStream_t stream) {
  const uint32_t G = lnx::slice_grid(n, kEpBlock, kEpGridCap);
  const RstCfg c = lnxr::rst_cfg_of(cfg);
  const uint4* rb = reinterpret_cast<const uint4*>(rec);
  hipError_t e;
  hipLaunchKernelGGL(echo_count_kernel, dim3(G), dim3(kEpBlock), 0, stream, bytes, off, n, trim, rb, c.fcs, ws);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(echo_scan_kernel, dim3(1), dim3(kEpGridCap), 0, stream, ws, G, cap, cap_blocks, d_n);
  if ((e = hipGetLastError()) != hipSuccess || cap == 0 || cap_blocks == 0) return e;
  return lnx::launch_fcs(c.fcs, echo_reply_kernel<true>, echo_reply_kernel<false>, dim3(G), dim3(kEpBlock), stream, bytes, off, n,
                         trim, rb, c, ip_id, cap, cap_blocks, ws, image, reinterpret_cast<uint32_t*>(reply), start, len, src, d_n);
}

}  // namespace lnxe
