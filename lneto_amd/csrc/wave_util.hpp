// wave_util.hpp — the small helpers every kernel file shares: byte masks of a
// loaded word, the RFC 1071 fold, and (device only) the DPP row reductions,
// the half-word dot product, a lane's rank and the wave prefix sum.  The first
// part is plain C++ that a host compiler also accepts (frame_plan.hpp,
// slice_walk.hpp and their host tests use it).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LNX_HD __host__ __device__ __forceinline__
#else
#define LNX_HD inline
#endif

namespace lnx {

// Bytes [lo, 4) of a little-endian word kept (lo clamped to 0..4).
LNX_HD uint32_t keep_from(int32_t lo) {
  lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
  return (uint32_t)(0xFFFFFFFFull << (8 * lo));
}
// byte mask of the frame offsets [a, b) inside the word whose byte 0 is at o0
LNX_HD uint32_t range_mask(int32_t o0, int32_t a, int32_t b) {
  return keep_from(a - o0) & ~keep_from(b - o0);
}
LNX_HD uint64_t keep8(int32_t d) {  // bytes [d, 8) of a qword, d clamped to 0..8
  const uint32_t q = 4u * (uint32_t)(d < 0 ? 0 : (d > 8 ? 8 : d));
  return (~0ull << q) << q;
}
LNX_HD uint16_t fold_sum16(uint32_t sum) {  // sum16, crc.go:17-21
  sum = (sum & 0xffffu) + (sum >> 16);
  return (uint16_t)~(uint16_t)(sum + (sum >> 16));
}

#if defined(__HIPCC__)
// acc + the two little-endian 16-bit halves of w (v_dot2_u32_u16)
__device__ __forceinline__ uint32_t dot2(uint32_t w, uint32_t acc) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 ones = {1, 1};
  return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, w), ones, acc, false);
}

// Sum / XOR over each 16-lane row, the result in every lane of the row.
__device__ __forceinline__ uint32_t row_add16(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false);  // row_ror:4
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
  return v;
}
__device__ __forceinline__ uint32_t row_xor16(uint32_t v) {
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false);
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false);
  return v;
}
// The least value of each 16-lane row, in every lane of the row.
__device__ __forceinline__ uint32_t row_min16(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false));
  return v;
}
// the XOR / sum over an 8-lane row (two quad steps, then the other quad of the half row)
__device__ __forceinline__ uint32_t row_xor8(uint32_t v) {
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
  return v;
}
__device__ __forceinline__ uint32_t row_add8(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false);
  return v;
}
// The four rows' sums joined in scalar registers (wave-uniform).
__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
  v = row_add16(v);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
         (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
// Among the wave's lanes with q set: those below this lane, and all of them (wave-uniform).
__device__ __forceinline__ void wave_rank(bool q, uint32_t& below, uint32_t& count) {
  const uint64_t m = __builtin_amdgcn_ballot_w64(q);
  below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  count = (uint32_t)__builtin_popcountll(m);
}
// An inclusive prefix sum over the wave's lanes.
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
    v += lane >= d ? o : 0u;
  }
  return v;
}

// A value every lane holds alike, moved to scalar registers so that the
// branches and loop bounds taken from it are scalar too.
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}
#endif  // __HIPCC__

}  // namespace lnx
