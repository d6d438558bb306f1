// slice_walk.hpp — the count / scan / walk-again shape of the delivery grouping
// and the reply kernels: G workgroups, each owning ONE
// contiguous index slice of whole chunks; a first launch counts per slice, one
// workgroup scans the counts in index order, and a last launch walks the same
// slices again, a chunk at a time, ranking each frame in its chunk
// (block_total, written_wanted and chunk_rank: the three launches' shared
// steps).  The first part is plain C++ that a host compiler also accepts
// (tests/cpp/slice_walk_host.cpp).
#pragma once
#include <cstdint>
#include "wave_util.hpp"

namespace lnx {

// The workgroups of the count and the walk launches over n frames in chunks of `block`.
LNX_HD uint32_t slice_grid(uint64_t n, uint32_t block, uint32_t cap) {
  const uint64_t chunks = (n + block - 1) / block;
  return (uint32_t)(chunks < cap ? (chunks ? chunks : 1) : cap);
}
// Workgroup g of G owns the index slice [lo, hi): `per` consecutive chunks of
// `block` frames, per = ceil(chunks / G); the last workgroups' slices may be
// short or empty.  Both launches use the same G.
LNX_HD void slice_bounds(uint64_t n, uint32_t block, uint32_t g, uint32_t G, uint64_t& lo, uint64_t& hi) {
  const uint64_t chunks = (n + block - 1) / block;
  const uint64_t per = (chunks + G - 1) / G;
  lo = (uint64_t)g * per * block;
  lo = lo < n ? lo : n;
  hi = lo + per * block;
  hi = hi < n ? hi : n;
}
// The length of the frame bytes[s : e] without its last `trim` bytes.
LNX_HD uint32_t frame_len(uint64_t s, uint64_t e, uint32_t trim) {
  const uint64_t lt = e > s ? e - s : 0;  // an end below its start: an empty frame
  const uint32_t Lt = lt < 0x7FFFFFFFull ? (uint32_t)lt : 0x7FFFFFFFu;
  return Lt > trim ? Lt - trim : 0u;
}
// What a scan launch reports of one sum: d_n[0] = the entries written, the first `cap` of them, d_n[1] = all of them.
LNX_HD void written_wanted(uint32_t* d_n, uint32_t total, uint64_t cap) {
  d_n[0] = total < cap ? total : (uint32_t)cap;
  d_n[1] = total;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void slice_bounds(uint64_t n, uint32_t block, uint64_t& lo, uint64_t& hi) {  // this workgroup's
  slice_bounds(n, block, blockIdx.x, gridDim.x, lo, hi);
}

// A frame's fields from its own aligned dwords only: a dword that holds a
// byte below L lies in that byte's page, so nothing else is loaded.
__device__ __forceinline__ uint32_t own_dword(const uint8_t* a) {
  return *reinterpret_cast<const uint32_t*>(reinterpret_cast<uintptr_t>(a) & ~(uintptr_t)3);
}
__device__ __forceinline__ uint32_t own_byte(const uint8_t* a) {
  return (own_dword(a) >> (8u * (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3u))) & 0xFFu;
}

// After the barrier behind the waves' stores of lds[wave]: the sum of the waves
// before `wave`, and of all kWaves.
template <uint32_t kWaves>
__device__ __forceinline__ void waves_before(const uint32_t* lds, uint32_t wave, uint32_t& before, uint32_t& total) {
  before = total = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w) {
    const uint32_t v = lds[w];
    before += w < wave ? v : 0u;
    total += v;
  }
}

// The Hillis-Steele inclusive scan over a workgroup of N threads, a value a
// thread, through an LDS array of N: two barriers a round.  Every thread of the
// workgroup calls it.  Several sums, each with an array of its own (ScanSlot),
// advance in the same rounds; v becomes the inclusive sum.
template <typename T>
struct ScanSlot {
  T* lds;
  T v, up;
};
template <uint32_t N, typename... T>
__device__ __forceinline__ void block_scan_inclusive(ScanSlot<T>&... s) {
  const uint32_t t = threadIdx.x;
  ((s.lds[t] = s.v), ...);
  __syncthreads();
  for (uint32_t d = 1; d < N; d <<= 1) {
    ((s.up = t >= d ? s.lds[t - d] : T{}), ...);
    __syncthreads();
    ((s.lds[t] += s.up), ...);
    __syncthreads();
  }
  ((s.v = s.lds[t]), ...);
}
template <uint32_t N, typename T>
__device__ __forceinline__ T block_scan_inclusive(T* lds, T v) {  // one sum
  ScanSlot<T> s{lds, v, T{}};
  block_scan_inclusive<N>(s);
  return s.v;
}

// The count launches' tail.  v: the wave's sum, in every lane of it; lds: an
// array of kWaves per sum.  Thread 0 leaves with the workgroup's sum in v (the
// other threads' v is not a sum).  One barrier; every thread of the workgroup calls it.
template <uint32_t kWaves, typename... T>
__device__ __forceinline__ void block_total(ScanSlot<T>&... s) {
  if ((threadIdx.x & 63u) == 0) ((s.lds[threadIdx.x >> 6] = s.v), ...);
  __syncthreads();
  if (threadIdx.x == 0) {
    ((s.v = T{}), ...);
    for (uint32_t w = 0; w < kWaves; ++w) ((s.v += s.lds[w]), ...);
  }
}

// A thread's rank in its chunk among the threads with q set, and the chunk's
// count of them: the waves' counts before its wave (through LDS, an array of
// kWaves per sum) plus the set lanes below it in its wave.  Two barriers,
// shared by all the sums of one call: the first also ends the last chunk's
// reads of whatever the caller stages by rank.  Every thread of the workgroup calls it.
struct RankSlot {
  uint32_t* lds;
  bool q;
  uint32_t rank, total;
};
template <uint32_t kWaves, typename... S>
__device__ __forceinline__ void chunk_rank(S&... s) {
  const uint32_t wave = threadIdx.x >> 6;
  (wave_rank(s.q, s.rank, s.total), ...);
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) ((s.lds[wave] = s.total), ...);
  __syncthreads();
  auto join = [wave](RankSlot& r) {
    uint32_t before;
    waves_before<kWaves>(r.lds, wave, before, r.total);
    r.rank += before;
  };
  (join(s), ...);
}
#endif  // __HIPCC__

}  // namespace lnx
