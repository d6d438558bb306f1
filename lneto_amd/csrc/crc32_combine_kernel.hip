// crc32_combine_kernel.hip — the running-crc forms of the batched CRC-32, gfx950:
// zlib's crc32_combine over pairs, the CRC32Update hook's crc argument, and
// frames made of segments.
//
// With Z_k = "advance the register over k zero bytes" (gf2.hpp),
//   CRC32Update(s, p) = CRC32(p) ^ Z_len(p)(s)
//   CRC32(A || B)     = Z_|B|(CRC32(A)) ^ CRC32(B)
// (the init / xorout inversions cancel), and for segments g_0..g_{m-1}
//   CRC32Update(s, g_0 || ... || g_{m-1}) = Z_total(s) ^ XOR_k Z_{suffix_k}(CRC32(g_k)),
// suffix_k = the bytes after g_k.  Every kernel here works on CRCs and lengths
// only; the bytes are read by the rows / staged / segment kernels, unchanged.
//
// Z_k for a 64-bit k is square-and-multiply over X_j = x^(8 * 2^j) mod P,
// j = 0..63: Z_k = the product of Z_{2^j} over the set bits j of k.  The
// multiply by the constant X_j is eight nibble lookups (no loop, no exit that
// depends on the data): kZImage holds Z_{2^j}(v << 4i) for every j, nibble
// position i and nibble v, built at compile time from gf2.hpp.  The levels of
// the low 32 length bits (16 KiB) are copied into the workgroup's LDS: a
// lookup's 16 entries lie in 16 banks and equal addresses broadcast, so the
// reads are conflict free.  Levels 32..63 (lengths of 4 GiB and up) are read
// from the image in global memory.
//
// The kernels live in namespace lnxc: the product library's lnx:: kernel list
// is pinned by tests/test_abi.py, this namespace's by tests/test_crc_chain.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gf2.hpp"
#include "launch.hpp"
#include "wave_util.hpp"

namespace lnxc {

using lnx::row_xor16;
using lnx::uniform64;

constexpr int kZLevels = 64;              // bits of a length
constexpr int kZDwords = kZLevels * 128;  // eight 16-entry nibble tables per level: 32 KiB
constexpr int kLdsLevels = 32;            // the levels held in LDS
constexpr int kLdsDwords = kLdsLevels * 128;

struct alignas(16) ZImage {
  uint32_t t[kZDwords];
};

// Entry (j, i, v) at dword 128 j + 16 i + v is X_j * (v << 4i) mod P.  Bit b of
// a reflected register is x^(31-b), so bit b-1 is bit b times x (zbit), and the
// rest is linearity.
constexpr ZImage make_zimage() {
  ZImage z{};
  uint32_t xj = lnx::x8kmodp(1);  // X_0 = x^8
  for (int j = 0; j < kZLevels; ++j) {
    uint32_t basis[32] = {};
    basis[31] = xj;  // X_j * x^0
    for (int b = 31; b > 0; --b) basis[b - 1] = lnx::zbit(basis[b]);
    for (int i = 0; i < 8; ++i)
      for (uint32_t v = 0; v < 16; ++v) {
        uint32_t e = 0;
        for (int q = 0; q < 4; ++q)
          if ((v >> q) & 1u) e ^= basis[4 * i + q];
        z.t[128 * j + 16 * i + v] = e;
      }
    xj = lnx::multmodp(xj, xj);  // X_{j+1} = X_j^2
  }
  return z;
}
constexpr ZImage kZHost = make_zimage();
static_assert(kZHost.t[128 * 0 + 16 * 7 + 8] == lnx::x8kmodp(1), "Z_1(x^0) = x^8");
static_assert(kZHost.t[128 * 37 + 16 * 7 + 8] == lnx::x8kmodp(1ull << 37), "level 37 is x^(8 * 2^37)");
static_assert(kZHost.t[128 * 63 + 16 * 2 + 5] == lnx::multmodp(lnx::x8kmodp(1ull << 63), 5u << 8), "level 63, nibble 2");
__device__ const ZImage kZImage = make_zimage();

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kResidue = 0x2144DF1Cu;  // LNX_CRC32_RESIDUE

struct alignas(16) ZLds {
  uint32_t t[kLdsDwords];
};

__device__ __forceinline__ void load_zimage(uint32_t* zt) {
  const uint4* src = reinterpret_cast<const uint4*>(kZImage.t);
  uint4* dst = reinterpret_cast<uint4*>(zt);
  static_assert(kLdsDwords / 4 % kBlock == 0, "a whole number of 16-byte loads per thread");
#pragma unroll
  for (uint32_t u = 0; u < kLdsDwords / 4 / kBlock; ++u) dst[threadIdx.x + u * kBlock] = src[threadIdx.x + u * kBlock];
  __syncthreads();
}

// OR over each 16-lane row, the result in every lane of the row (the DPP
// chain of wave_util.hpp's row_xor16).
__device__ __forceinline__ uint32_t row_or16(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false);  // row_ror:4
  v |= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false);  // row_ror:8
  return v;
}
// The four rows' values joined in scalar registers (wave-uniform).
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
  v = row_or16(v);
  return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) | __builtin_amdgcn_readlane((int)v, 16) |
                    __builtin_amdgcn_readlane((int)v, 32) | __builtin_amdgcn_readlane((int)v, 48));
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
  v = row_xor16(v);
  return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) ^ __builtin_amdgcn_readlane((int)v, 16) ^
                    __builtin_amdgcn_readlane((int)v, 32) ^ __builtin_amdgcn_readlane((int)v, 48));
}

// Z_{2^j}(r), zl = the level's eight nibble tables.
__device__ __forceinline__ uint32_t zlevel(const uint32_t* zl, uint32_t r) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) x ^= zl[16 * i + ((r >> (4 * i)) & 15u)];
  return x;
}

// Z_k(r) with a k of its own in every lane.  Call it with the whole wave
// active: the loop runs over the bits set in ANY lane's k (a scalar mask, so
// its trip count is wave-uniform and no lane leaves early); a lane whose k
// lacks the bit keeps its r.  Nothing is looked up when every lane's r is 0.
__device__ __forceinline__ uint32_t zpow(const uint32_t* zt, uint32_t r, uint64_t k) {
  if (wave_or(r) == 0u) return r;
  const uint32_t klo = (uint32_t)k, khi = (uint32_t)(k >> 32);
  uint32_t mlo = wave_or(klo), mhi = wave_or(khi);
  while (mlo) {  // levels 0..31, in LDS
    const int j = __builtin_ctz(mlo);
    mlo &= mlo - 1;
    const uint32_t t = zlevel(zt + 128 * j, r);
    r = ((klo >> j) & 1u) ? t : r;
  }
  while (mhi) {  // levels 32..63, from the image in global memory
    const int j = __builtin_ctz(mhi);
    mhi &= mhi - 1;
    const uint32_t t = zlevel(kZImage.t + 128 * (kLdsLevels + j), r);
    r = ((khi >> j) & 1u) ? t : r;
  }
  return r;
}

enum class PairMode : int { kCombine = 0, kSeed = 1 };

// One lane per pair.
//   kCombine: out[i] = Z_{len[i]}(a[i]) ^ b[i]               (lnx_crc32_combine_batch; out may alias a or b)
//   kSeed:    out[i] ^= Z_{len_i}(a[i]), len_i = off[i+1] - off[i] clamped at 0, off = `len`
//             (lnx_crc32_update_batch after lnx_crc32_batch's launches; a = the seeds)
// The grid-stride loop's trip count is uniform over the workgroup; lanes past
// n read pair n - 1 and store nothing.
template <PairMode MODE>
__global__ void __launch_bounds__(kBlock)
combine_pairs_kernel(const uint32_t* a, const uint32_t* b, const uint64_t* len, uint64_t n, uint32_t* out) {
  __shared__ ZLds zs;
  load_zimage(zs.t);
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += stride) {
    const uint64_t i = base + threadIdx.x;
    const bool live = i < n;
    const uint64_t ii = live ? i : n - 1;
    uint32_t r = a[ii], x;
    uint64_t k;
    if constexpr (MODE == PairMode::kSeed) {
      const uint64_t s = len[ii], e = len[ii + 1];
      k = e > s ? e - s : 0ull;
      x = out[ii];
    } else {
      k = len[ii];
      x = b[ii];
    }
    r = zpow(zs.t, r, k) ^ x;
    if (live) out[i] = r;
  }
}

// Inclusive suffix sum over each `W`-lane group (W = 16 or 64).
template <int W>
__device__ __forceinline__ uint64_t suffix_sum(uint64_t v, uint32_t p) {
#pragma unroll
  for (int d = 1; d < W; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d, W);
    const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d, W);
    v += p + d < (uint32_t)W ? ((uint64_t)hi << 32 | lo) : 0ull;
  }
  return v;
}

// A row's frames of up to kRowSegs segments are folded by the row; longer
// frames by the whole workgroup, one after the other.
constexpr uint64_t kRowSegs = 256;  // 16 lanes x 16 segments

// Segments [a, b) folded in order from `acc`: acc = Z_len(acc) ^ crc per
// segment, L = their bytes.  `steps` is uniform over the wave (>= b - a); a
// lane past its run folds the identity (length 0, CRC 0) of segment 0.
__device__ __forceinline__ void fold_run(const uint32_t* zt, const uint32_t* seg_crc, const uint32_t* len, uint64_t a,
                                         uint64_t b, uint64_t steps, uint32_t& acc, uint64_t& L) {
  constexpr int kAhead = 8;  // segments loaded before the first of them is folded
  for (uint64_t t0 = 0; t0 < steps; t0 += kAhead) {
    uint32_t x[kAhead], l[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const uint64_t idx = a + t0 + u;
      const bool lv = idx < b;
      const uint64_t ic = lv ? idx : 0ull;
      x[u] = seg_crc[ic], l[u] = len[ic];
      x[u] = lv ? x[u] : 0u, l[u] = lv ? l[u] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (t0 + u < steps) {  // uniform over the wave
        acc = zpow(zt, acc, l[u]) ^ x[u];
        L += l[u];
      }
    }
  }
}

// Frame f = segments min(first[f], nseg) .. min(first[f+1], nseg) - 1 in index
// order; seg_crc / len = each segment's own CRC and length.
//   out[f] = Z_total(seed[f]) ^ XOR_k Z_{suffix_k}(seg_crc[k])        (VERIFY: out[f] = that == residue, total >= 4)
// One 16-lane row per frame, sixteen frames per workgroup pass: lane p folds a
// contiguous run of ceil(m / 16) segments in order (the loop runs to the
// wave's largest run), the row's suffix sum of the runs' bytes gives each lane
// the bytes after its run, one Z over that and a row XOR join the lanes.  A
// frame of more than kRowSegs segments is folded the same way by the
// workgroup's 256 lanes, the waves joined through LDS.
template <bool VERIFY>
__global__ void __launch_bounds__(kBlock)
chain_fold_kernel(const uint32_t* __restrict__ seg_crc, const uint32_t* __restrict__ len, uint64_t nseg,
                  const uint64_t* __restrict__ first, uint64_t nframes, const uint32_t* __restrict__ seed,
                  void* __restrict__ out) {
  __shared__ ZLds zs;
  __shared__ uint64_t big_s0[16], big_m[16], wave_len[kWaves];
  __shared__ uint32_t big_seed[16], wave_acc[kWaves];
  load_zimage(zs.t);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, p = lane & 15u, wave = tid >> 6, slot = tid >> 4;
  auto store = [&](uint64_t f, uint32_t crc, uint64_t total) {
    if constexpr (VERIFY)
      static_cast<uint8_t*>(out)[f] = (uint8_t)(total >= 4 && crc == kResidue);
    else
      static_cast<uint32_t*>(out)[f] = crc;
  };
  const uint64_t stride = (uint64_t)gridDim.x * 16;
  for (uint64_t f0 = (uint64_t)blockIdx.x * 16; f0 < nframes; f0 += stride) {
    const uint64_t f = f0 + slot;
    const bool live = f < nframes;
    const uint64_t ff = live ? f : nframes - 1;
    const uint64_t s0 = min(first[ff], nseg), s1 = min(first[ff + 1], nseg);
    const uint64_t m = live && s1 > s0 ? s1 - s0 : 0ull;
    const uint32_t sd = !VERIFY && seed ? seed[ff] : 0u;
    const bool big = m > kRowSegs;
    if (p == 0) big_s0[slot] = s0, big_m[slot] = big ? m : 0ull, big_seed[slot] = sd;
    // (also the barrier between the lines above and the workgroup's reads below)
    const bool any_big = __builtin_amdgcn_readfirstlane(__syncthreads_or((int)big)) != 0;
    {
      const uint64_t mr = big ? 0ull : m;
      const uint32_t c = (uint32_t)((mr + 15) >> 4);  // the row's run length
      const uint32_t cw = max(max((uint32_t)__builtin_amdgcn_readlane((int)c, 0), (uint32_t)__builtin_amdgcn_readlane((int)c, 16)),
                              max((uint32_t)__builtin_amdgcn_readlane((int)c, 32), (uint32_t)__builtin_amdgcn_readlane((int)c, 48)));
      const uint64_t a = s0 + (uint64_t)p * c, b = min(a + c, s0 + mr);
      uint32_t acc = p == 0 ? sd : 0u;
      uint64_t L = 0;
      fold_run(zs.t, seg_crc, len, a, b, cw, acc, L);
      const uint64_t S = suffix_sum<16>(L, p);  // bytes of this run and the runs after it
      acc = row_xor16(zpow(zs.t, acc, S - L));
      const uint32_t tl = (uint32_t)__shfl((int)(uint32_t)S, 0, 16), th = (uint32_t)__shfl((int)(uint32_t)(S >> 32), 0, 16);
      if (live && !big && p == 0) store(f, acc, (uint64_t)th << 32 | tl);
    }
    if (!any_big) continue;  // uniform over the workgroup
    for (uint32_t q = 0; q < 16; ++q) {
      const uint64_t M = uniform64(big_m[q]);
      if (M == 0) continue;  // uniform over the workgroup
      const uint64_t S0 = uniform64(big_s0[q]), c = (M + kBlock - 1) / kBlock;
      const uint64_t a = min(S0 + (uint64_t)tid * c, S0 + M), b = min(a + c, S0 + M);
      uint32_t acc = tid == 0 ? big_seed[q] : 0u;
      uint64_t L = 0;
      fold_run(zs.t, seg_crc, len, a, b, c, acc, L);
      uint64_t S = suffix_sum<64>(L, lane);
      const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)S, 0),
                     wh = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(S >> 32), 0);
      if (lane == 0) wave_len[wave] = (uint64_t)wh << 32 | wl;
      __syncthreads();
      uint64_t total = 0;
#pragma unroll
      for (uint32_t w = 0; w < kWaves; ++w) {
        total += wave_len[w];
        S += w > wave ? wave_len[w] : 0ull;  // the waves after this one
      }
      acc = wave_xor(zpow(zs.t, acc, S - L));
      if (lane == 0) wave_acc[wave] = acc;
      __syncthreads();
      if (tid == 0) store(f0 + q, wave_acc[0] ^ wave_acc[1] ^ wave_acc[2] ^ wave_acc[3], total);
    }
    __syncthreads();  // big_* and wave_* are rewritten by the next pass
  }
}

namespace {
// 16 KiB of LDS and four waves per workgroup: eight fill a CU's 32 wave slots
// (the cap is restated in tests/test_grid_passes.py LAUNCH).
unsigned grid_for(uint64_t items, uint64_t per_block, int num_cus) {
  const uint64_t want = (items + per_block - 1) / per_block, cap = (uint64_t)(num_cus > 0 ? num_cus : 1) * 8;
  return (unsigned)(want < cap ? want : cap);
}
}  // namespace

hipError_t launch_combine_pairs(const uint32_t* a, const uint32_t* b, const uint64_t* len, uint64_t n, uint32_t* out,
                                int num_cus, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(combine_pairs_kernel<PairMode::kCombine>, dim3(grid_for(n, kBlock, num_cus)), dim3(kBlock), 0,
                     stream, a, b, len, n, out);
  return hipGetLastError();
}

hipError_t launch_seed_pairs(const uint32_t* seed, const uint64_t* off, uint64_t n, uint32_t* crc, int num_cus,
                             hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(combine_pairs_kernel<PairMode::kSeed>, dim3(grid_for(n, kBlock, num_cus)), dim3(kBlock), 0,
                     stream, seed, static_cast<const uint32_t*>(nullptr), off, n, crc);
  return hipGetLastError();
}

hipError_t launch_chain_fold(const uint32_t* seg_crc, const uint32_t* len, uint64_t nseg, const uint64_t* first,
                             uint64_t nframes, const uint32_t* seed, void* out, bool verify, int num_cus,
                             hipStream_t stream) {
  if (nframes == 0) return hipSuccess;
  const dim3 grid(grid_for(nframes, 16, num_cus));
  if (verify)
    hipLaunchKernelGGL(chain_fold_kernel<true>, grid, dim3(kBlock), 0, stream, seg_crc, len, nseg, first, nframes,
                       static_cast<const uint32_t*>(nullptr), out);
  else
    hipLaunchKernelGGL(chain_fold_kernel<false>, grid, dim3(kBlock), 0, stream, seg_crc, len, nseg, first, nframes,
                       seed, out);
  return hipGetLastError();
}

}  // namespace lnxc
