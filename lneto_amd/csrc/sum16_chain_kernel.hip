// sum16_chain_kernel.hip — the running forms of the batched internet checksum
// (lneto CRC791, crc.go:13-62), gfx950: the raw 32-bit sum of a segment at
// either byte phase of its packet, and frames made of segments.
//
// With E_k / O_k = the sums of segment k's bytes at even / odd offsets from its
// own start and pos_k = the bytes before it in its frame, the reference's
// 32-bit value before sum16 (crc.go:17-21) is
//   S(s, g_0 || ... || g_{m-1}) = s + SUM_k (pos_k even ? 256 E_k + O_k : E_k + 256 O_k)   (mod 2^32)
// (sumWriteEven's big-endian words, crc.go:23-28; the `<< 8` of an odd last
// byte, crc.go:56).  Everything is linear mod 2^32, so the reference's own
// wrap-around is reproduced exactly: no 64-bit accumulator and no end-around
// carry before the last fold.  Only pos_k & 1 matters, the terms commute, and
// E_k, O_k may themselves be taken mod 2^32.
//
// The kernels live in namespace lnxs: the product library's lnx:: kernel list
// is pinned by tests/test_abi.py, this namespace's by tests/test_sum_chain.py.
// The row helpers shared with sum16_kernel.hip are wave_util.hpp's.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.hpp"
#include "wave_util.hpp"

namespace lnxs {

using lnx::fold_sum16;
using lnx::keep8;
using lnx::row_add16;
using lnx::uniform64;
using lnx::wave_add;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kLineUnroll = 13;  // lines per row in flight (sum16_kernel.hip kLineUnroll)

enum class ByteMode : int { kPlanes = 0, kPartial = 1 };

// The line rows of sum16_lines_kernel (sum16_kernel.hip: a 16-lane row per
// segment, 8 bytes a lane so that a row instruction reads one whole 128-byte
// line, kLineUnroll lines in flight, the first line and the last two at the
// default cache policy and the rest non-temporal, v_dot4_u32_u8 with the
// weights picked by the start's parity), with the raw sums as results:
//   kPlanes:  out[i] = E_i, out[nseg + i] = O_i              (lnx_sum16_chain_batch's workspace)
//   kPartial: out[i] = seed[i] + (phase[i] & 1 ? E_i + 256 O_i : 256 E_i + O_i)   (lnx_sum_partial_batch)
// One wave-uniform loop to the wave's largest line count: a loop with per-row
// exits around the dwordx2 loads is the shape DESIGN.md §3.2 records returning
// wrong sums on this chip.
template <ByteMode MODE>
__global__ void __launch_bounds__(kBlock)
sum_bytes_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                 const uint32_t* __restrict__ seed, const uint8_t* __restrict__ phase, uint64_t nseg,
                 uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u, p = lane & 15u, row = lane >> 4;
  const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t q = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); q * 4 < nseg; q += nwaves) {
    const uint64_t i = q * 4 + row;
    const bool live = i < nseg;
    const uint64_t s = live ? off[i] : 0;
    const uint32_t L = live ? len[i] : 0u;
    uint32_t sd = 0, ph = 0;
    if constexpr (MODE == ByteMode::kPartial) {
      sd = live && seed ? seed[i] : 0u;
      ph = live && phase ? (uint32_t)phase[i] & 1u : 0u;
    }
    const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(bytes) + s) & 127u);
    const uint64_t* base = reinterpret_cast<const uint64_t*>(bytes + s - mis) + p;
    const uint32_t nl = L ? (mis + L + 127u) >> 7 : 0u;  // lines touching the segment
    // bytes at even segment offsets sit at positions {0,2} of a dword when the
    // segment starts 2-aligned, {1,3} otherwise
    const uint32_t wE = (mis & 1u) ? 0x01000100u : 0x00010001u;
    const uint32_t wO = (mis & 1u) ? 0x00010001u : 0x01000100u;
    uint32_t E = 0, O = 0;
    uint32_t nlw = max(nl, (uint32_t)__shfl_xor((int)nl, 16));
    nlw = max(nlw, (uint32_t)__shfl_xor((int)nlw, 32));
    nlw = (uint32_t)__builtin_amdgcn_readfirstlane((int)nlw);
    for (uint32_t k0 = 0; k0 < nlw; k0 += kLineUnroll) {
      uint64_t x[kLineUnroll];
#pragma unroll
      for (int u = 0; u < kLineUnroll; ++u) {
        const bool nt = !(u == 0 || u >= kLineUnroll - 2);
        x[u] = k0 + u < nl ? (nt ? __builtin_nontemporal_load(base + 16u * (k0 + u)) : base[16u * (k0 + u)]) : 0ull;
      }
#pragma unroll
      for (int u = 0; u < kLineUnroll; ++u) {
        const int32_t o0 = (int32_t)(128u * (k0 + u) + 8u * p) - (int32_t)mis;  // segment offset of byte 0
        const uint64_t y = x[u] & keep8(-o0) & ~keep8((int32_t)L - o0);
        E = __builtin_amdgcn_udot4((uint32_t)y, wE, E, false);
        O = __builtin_amdgcn_udot4((uint32_t)y, wO, O, false);
        E = __builtin_amdgcn_udot4((uint32_t)(y >> 32), wE, E, false);
        O = __builtin_amdgcn_udot4((uint32_t)(y >> 32), wO, O, false);
      }
    }
    E = row_add16(E);
    O = row_add16(O);
    if constexpr (MODE == ByteMode::kPartial) {
      if (live && p == 0) out[i] = sd + (ph ? E + 256u * O : 256u * E + O);
    } else {
      if (live && p == 0) out[i] = E;
      if (live && p == 1) out[nseg + i] = O;
    }
  }
}

// A row's frames of up to kRowSegs segments are folded by the row; longer
// frames by the whole workgroup, one after the other.
constexpr uint64_t kRowSegs = 256;  // 16 lanes x 16 segments
// Frames a row folds in one pass: their loads are in flight together (with one
// frame per row a pass of 1-segment frames waited out one round trip for 12
// bytes a row: 0.070 ms for 1 Mi frames).
constexpr int kRowFrames = 4;
constexpr int kPassFrames = 16 * kRowFrames;  // frames a workgroup takes per pass
constexpr int kAhead = 8;                     // steps of a long frame loaded before the first of them is summed

// Frame f = segments min(first[f], nseg) .. min(first[f+1], nseg) - 1 in index
// order; eo = the E plane [0, nseg) and the O plane [nseg, 2 nseg).
//   raw[f] = seed[f] + SUM_k (pos_k even ? 256 E_k + O_k : E_k + 256 O_k);  out16[f] = sum16(raw[f])
// One 16-lane row per frame, sixteen rows per workgroup, kRowFrames frames per
// row and pass (frame f0 + 16 u + row of the pass at f0, u < kRowFrames).  The
// terms commute, so lane p takes segments p, p + 16, ... of its frame
// (coalesced dword loads at clamped indices, the loop running to the wave's
// largest trip count).  A segment's phase is the frame's running parity bit
// XOR the parity of the odd lengths its row's lower lanes hold in that step,
// read from the row's 16 bits of a wave ballot.  A frame of more than kRowSegs
// segments is folded by the workgroup's four waves, a contiguous quarter each:
// a wave sums its quarter under both phases it may start at (the two differ by
// swapped weights), and one lane picks per wave by the parity of the quarters
// before it, through LDS.  No lane ever walks a long frame alone.  The next
// pass's d_first pairs are loaded before this pass's segments.
__global__ void __launch_bounds__(kBlock)
sum_fold_kernel(const uint32_t* __restrict__ eo, const uint32_t* __restrict__ len, uint64_t nseg,
                const uint64_t* __restrict__ first, uint64_t nframes, const uint32_t* __restrict__ seed,
                uint16_t* __restrict__ out16, uint32_t* __restrict__ sum32) {
  __shared__ uint64_t big_s0[kPassFrames], big_m[kPassFrames];
  __shared__ uint32_t big_seed[kPassFrames], wave_even[kWaves], wave_odd[kWaves], wave_par[kWaves];
  // byte `slot` of row_big[pass & 1]: bit u = the row's frame u is a long one.  Two copies, so that a wave
  // already in the next pass does not write the bytes a slower wave still reads (one barrier per pass).
  __shared__ uint4 row_big[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, p = lane & 15u, row = lane >> 4, wave = tid >> 6, slot = tid >> 4;
  const uint32_t* __restrict__ ev = eo;
  const uint32_t* __restrict__ od = eo + nseg;
  auto store = [&](uint64_t f, uint32_t raw) {
    if (out16) out16[f] = fold_sum16(raw);
    if (sum32) sum32[f] = raw;
  };
  const uint64_t stride = (uint64_t)gridDim.x * kPassFrames;
  uint64_t f0 = (uint64_t)blockIdx.x * kPassFrames;
  uint64_t na[kRowFrames], nb[kRowFrames];
#pragma unroll
  for (int u = 0; u < kRowFrames; ++u) {
    const uint64_t nf = min(f0 + 16u * u + slot, nframes - 1);  // nframes >= 1 (the launcher)
    na[u] = first[nf], nb[u] = first[nf + 1];
  }
  for (uint32_t pass = 0; f0 < nframes; f0 += stride, pass ^= 1u) {
    uint64_t s0[kRowFrames];
    uint32_t mr[kRowFrames], sd[kRowFrames], acc[kRowFrames], par[kRowFrames];
    uint32_t c = 0, wr = 0, bgm = 0;  // the row's steps; bit u: frame u is the row's to store / a long one
#pragma unroll
    for (int u = 0; u < kRowFrames; ++u) {
      const uint64_t f = f0 + 16u * u + slot;
      const bool live = f < nframes;
      s0[u] = min(na[u], nseg);
      const uint64_t s1 = min(nb[u], nseg);
      const uint64_t nf = min(f + stride, nframes - 1);
      na[u] = first[nf], nb[u] = first[nf + 1];
      const uint64_t m = live && s1 > s0[u] ? s1 - s0[u] : 0ull;
      sd[u] = live && seed ? seed[f] : 0u;
      const bool bg = m > kRowSegs;
      if (bg && p == 0) big_s0[16 * u + slot] = s0[u], big_m[16 * u + slot] = m, big_seed[16 * u + slot] = sd[u];
      mr[u] = bg ? 0u : (uint32_t)m;
      c = max(c, (mr[u] + 15u) >> 4);
      wr |= (uint32_t)(live && !bg) << u;
      bgm |= (uint32_t)bg << u;
      acc[u] = 0, par[u] = 0;  // par: the parity of the frame's bytes in the steps before this one
    }
    if (p == 0) reinterpret_cast<uint8_t*>(&row_big[pass])[slot] = (uint8_t)bgm;
    __syncthreads();
    const uint4 rb = row_big[pass];
    const bool any_big = __builtin_amdgcn_readfirstlane((int)(rb.x | rb.y | rb.z | rb.w)) != 0;
    const uint32_t cw = max(max((uint32_t)__builtin_amdgcn_readlane((int)c, 0), (uint32_t)__builtin_amdgcn_readlane((int)c, 16)),
                            max((uint32_t)__builtin_amdgcn_readlane((int)c, 32), (uint32_t)__builtin_amdgcn_readlane((int)c, 48)));
    for (uint32_t t = 0; t < cw; ++t) {
      const uint32_t j = 16u * t + p;
      uint32_t e[kRowFrames], o[kRowFrames], l[kRowFrames];
#pragma unroll
      for (int u = 0; u < kRowFrames; ++u) {
        const uint64_t ic = j < mr[u] ? s0[u] + j : 0ull;  // index 0 exists: cw > 0 only with nseg > 0
        e[u] = ev[ic], o[u] = od[ic], l[u] = len[ic];
      }
#pragma unroll
      for (int u = 0; u < kRowFrames; ++u) {
        const bool lv = j < mr[u];
        const uint32_t ee = lv ? e[u] : 0u, oo = lv ? o[u] : 0u, ll = lv ? l[u] : 0u;
        const uint32_t odd = (uint32_t)(__ballot((int)(ll & 1u)) >> (16u * row)) & 0xFFFFu;  // the row's odd lengths
        const uint32_t ph = (par[u] ^ (uint32_t)__popc(odd & ((1u << p) - 1u))) & 1u;
        acc[u] += ph ? ee + 256u * oo : 256u * ee + oo;
        par[u] ^= (uint32_t)__popc(odd) & 1u;
      }
    }
#pragma unroll
    for (int u = 0; u < kRowFrames; ++u) {
      const uint32_t r = row_add16(acc[u]);
      if (((wr >> u) & 1u) && p == 0) store(f0 + 16u * u + slot, sd[u] + r);
    }
    if (!any_big) continue;  // uniform over the workgroup
    for (uint32_t q = 0; q < (uint32_t)kPassFrames; ++q) {
      const uint32_t bits = reinterpret_cast<const uint8_t*>(&row_big[pass])[q & 15u];
      if (!__builtin_amdgcn_readfirstlane((int)((bits >> (q >> 4)) & 1u))) continue;  // uniform over the workgroup
      const uint64_t M = uniform64(big_m[q]);
      const uint64_t S0 = uniform64(big_s0[q]), cq = (M + kWaves - 1) / kWaves;  // a wave's quarter
      const uint64_t a = min((uint64_t)wave * cq, M), b = min(a + cq, M);
      const uint64_t steps = (cq + 63) >> 6;  // uniform over the workgroup
      uint32_t even = 0, oddsum = 0, wpar = 0;  // the quarter's sum if it starts at an even / odd offset
      for (uint64_t t0 = 0; t0 < steps; t0 += kAhead) {
        uint32_t e[kAhead], o[kAhead], l[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const uint64_t j = a + 64u * (t0 + u) + lane;
          const uint64_t ic = j < b ? S0 + j : 0ull;
          e[u] = ev[ic], o[u] = od[ic], l[u] = len[ic];
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {  // a step past the quarter's end holds zeros: nothing added, no parity
          const bool lv = a + 64u * (t0 + u) + lane < b;
          const uint32_t ee = lv ? e[u] : 0u, oo = lv ? o[u] : 0u, ll = lv ? l[u] : 0u;
          const uint64_t odd = __ballot((int)(ll & 1u));
          const uint32_t ph = (wpar ^ (uint32_t)__popcll(odd & ((1ull << lane) - 1ull))) & 1u;
          const uint32_t x = 256u * ee + oo, y = ee + 256u * oo;
          even += ph ? y : x;
          oddsum += ph ? x : y;
          wpar ^= (uint32_t)__popcll(odd) & 1u;
        }
      }
      even = wave_add(even);
      oddsum = wave_add(oddsum);
      if (lane == 0) wave_even[wave] = even, wave_odd[wave] = oddsum, wave_par[wave] = wpar;
      __syncthreads();
      if (tid == 0) {
        uint32_t raw = big_seed[q], ph = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
          raw += ph ? wave_odd[w] : wave_even[w];
          ph ^= wave_par[w];
        }
        store(f0 + q, raw);
      }
      __syncthreads();  // wave_* are rewritten by the next long frame
    }
    __syncthreads();  // big_* are rewritten by a later pass
  }
}

// lnx_sum_partial_batch / the first launch of lnx_sum16_chain_batch.  The grid
// is capped as launch_sum16_segments caps sum16_lines_kernel's: 256 workgroups
// of 16 segments per CU (the cap is restated in tests/test_sum_chain_gpu.py LAUNCH).
hipError_t launch_sum_bytes(const uint8_t* bytes, const uint64_t* off, const uint32_t* len, const uint32_t* seed,
                            const uint8_t* phase, uint64_t n, uint32_t* out, bool planes, int num_cus,
                            hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t seg_per_block = kWaves * 4;
  uint64_t grid = (n + seg_per_block - 1) / seg_per_block;
  const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * 256;
  if (grid > cap) grid = cap;
  if (planes)
    hipLaunchKernelGGL(sum_bytes_kernel<ByteMode::kPlanes>, dim3((unsigned)grid), dim3(kBlock), 0, stream, bytes, off,
                       len, static_cast<const uint32_t*>(nullptr), static_cast<const uint8_t*>(nullptr), n, out);
  else
    hipLaunchKernelGGL(sum_bytes_kernel<ByteMode::kPartial>, dim3((unsigned)grid), dim3(kBlock), 0, stream, bytes, off,
                       len, seed, phase, n, out);
  return hipGetLastError();
}

// Four waves, 79 vector registers and under 2 KiB of LDS per workgroup: six
// waves fit a SIMD, so six workgroups fill a CU, and the grid is capped at
// that (the cap is restated in tests/test_sum_chain_gpu.py LAUNCH).
hipError_t launch_sum_fold(const uint32_t* eo, const uint32_t* len, uint64_t nseg, const uint64_t* first,
                           uint64_t nframes, const uint32_t* seed, uint16_t* out16, uint32_t* sum32, int num_cus,
                           hipStream_t stream) {
  if (nframes == 0) return hipSuccess;
  const uint64_t want = (nframes + kPassFrames - 1) / kPassFrames, cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * 6;
  hipLaunchKernelGGL(sum_fold_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(kBlock), 0, stream, eo, len, nseg,
                     first, nframes, seed, out16, sum32);
  return hipGetLastError();
}

}  // namespace lnxs
