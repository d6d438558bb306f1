// stage_kernel.hip — batched CRC-32 / FCS verify by staged lane streams, gfx950
// (round 4, the product form since round 5).
// Reference semantics: ethernet.CRC32 (lneto ethernet/crc.go:19-21) =
// Go crc32.Checksum(data, IEEETable); the verify mode is the residue form of
// the FCS check.  The schedule is restated on the host in
// tests/stage_algebra.py and checked there against zlib.
//
// Why: on mixed-length frames (the Zipf mix, mean 246 B) every per-frame
// window layout is bound by the L2 request rate (a line two frames share is
// asked for twice, a short frame's partial lines cost a request each;
// DESIGN.md §4).  Here each line is requested once, whole, and a lane still
// folds a CONTIGUOUS byte stream, so a frame boundary costs no cross-lane work:
//
//  * a wave takes a block of kStageBF consecutive frames, bytes [A, E), and
//    cuts 64 stretches of Q bytes (Q a multiple of 128) from A rounded down to
//    128; lane k folds stretch k eight bytes at a time through lane-private
//    slicing-by-8 tables, r <- Z8(r ^ w0) ^ Z4(w1);
//  * per round each lane needs its stretch's next 128-byte line: 8
//    buffer_load_dwordx4, instruction m / lane t reading piece
//    ((t & 7) - s) & 7 of stretch s = 8 (t >> 3) + m, so every instruction
//    covers 8 whole lines; the pieces go to the wave's 8 KiB of LDS at
//    1024 m + 16 t and lane s reads its line back with 8 ds_read_b128 at
//    1024 (s & 7) + 128 (s >> 3) + 16 ((i + s) & 7), conflict-free;
//  * a boundary x (an offset of the block) in the dword at 4d, byte c:
//    e = r ^ (w & lomask(c)), the ending frame's state is Z_c(e) (its CRC the
//    complement); the new frame's chain starts from the patched word
//    (w & ~lomask(c)) ^ K_c, K_c = Z_{-c}(~0).  One boundary per 64-byte half
//    is handled inside the fold; a half where some lane has two (frames under
//    64 bytes, empty frames) runs byte by byte;
//  * a stretch starts inside a frame: its first boundary's state is local.
//    After the block, P_k (the true register at stretch k's start) is the
//    previous lane's end register (or, past a frame longer than a stretch,
//    Z_Q(P_{k-1}) ^ E_{k-1}), and the first frame's state gains Z_d(P_k),
//    d = x - S_k, by binary powers Z_{2^m} from shared nibble tables.
//
// Round 5: the kernel is the second launch behind the plain
// entries.  A workgroup folds its slice only when dispatch.hpp's slice_kind()
// gives it to this kernel; every workgroup then folds its share of the giant
// slices (bytes past 31-bit buffer offsets) in byte pieces, one piece per
// lane, the parts of a frame that crosses pieces joined by Z_d shifts and
// device-scope XORs into a per-stream scratch (giant_pieces below).  A block
// whose offsets are out of order is folded one lane per frame (ooo_block).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dispatch.hpp"
#include "launch.hpp"
#include "table_layout.hpp"

namespace lnx {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

enum class StageMode : int { kCrc = 0, kVerify = 1 };

constexpr uint32_t kStageBF = 382;  // frames per block: the boundary list (bf + 1 + 2 sentinels) fits 384 dwords
constexpr uint32_t kStageW = 8;     // waves per workgroup (two per SIMD: 182-193 VGPRs each)
// LDS layout (bytes)
constexpr uint32_t kSTab = 0;                          // T8_k tables: e << 8 | k << 5 | c << 2 (64 KiB)
constexpr uint32_t kSList = (kStageBF + 2) * 4;         // boundary list bytes per wave
constexpr uint32_t kSTr = 65536;                        // transposes: 8 KiB per wave
constexpr uint32_t kSBnd = kSTr + kStageW * 8192;       // boundary lists
constexpr uint32_t kSNib = kSBnd + kStageW * kSList;    // Z_{2^m}, m = 0..30: (m, i, v) at 512 m + 64 i + 4 v
constexpr uint32_t kSCtr = kSNib + 31 * 512;            // the workgroup's block counter
constexpr uint32_t kSGpre = kSCtr + 16;                 // giant slices: frame prefix gpre[0..G] (G <= 256)
constexpr uint32_t kSBad = kSGpre + 260 * 4;            // giant slices out of order: bit g of 8 dwords
constexpr uint32_t kSBytes = kSBad + 32;
static_assert(kSBytes <= 163840, "stage LDS");
static_assert((kStageBF + 2) % 64 == 0, "whole-wave list loads");
// (the image in HBM: table_layout.hpp kStageZ8Img, kStageNibImg, kStageNibHiImg)
// giant slices: pieces of at least this many bytes, at most kGiantPieces of them
constexpr uint64_t kGiantPieceMin = 16384;
constexpr uint32_t kGiantPieces = 1u << 20;

constexpr uint32_t kSOOB = 0x80000000u;
constexpr uint32_t kSNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t s_lds(const char* lds, uint32_t a) {
  return *reinterpret_cast<const uint32_t*>(lds + a);
}
// Z_1(v): the T8_7 table
__device__ __forceinline__ uint32_t s_z1(const char* lds, uint32_t v, uint32_t b0) {
  return (v >> 8) ^ s_lds(lds, kSTab + __builtin_amdgcn_perm(v, b0, 0x0c020400u) + 224u);
}
// Slicing-by-8 over 8-byte units, the eight byte tables T8_k[e] = Z_{8-k}(e)
// in 8 bank columns, entry e of table k, column c at e << 8 | k << 5 | c << 2
// (64 KiB).  A unit (w0, w1) entered with r leaves Z_8(r ^ w0) ^ Z_4(w1) =
// XOR_k T8_k[byte k of r ^ w0] ^ XOR_k T8_{4+k}[byte k of w1]: the w1 half is
// off the chain, so a lane's chain takes one LDS round trip per 8 bytes.
// Table k sits in bank octet k & 3; the four 8-lane groups g = (lane >> 3) & 3
// of a pass read tables (i + g) & 3 (and 4 + that) in lookup i, so each
// lookup instruction is conflict-free.
struct Z8Lane {
  uint32_t base[8], sel[4];  // base[i] (table (i + g) & 3), base[4 + i] (table 4 + ((i + g) & 3))
  __device__ explicit Z8Lane(uint32_t lane) {
    const uint32_t g = (lane >> 3) & 3u, c = lane & 7u;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t k = (i + g) & 3u;
      base[i] = (k << 5) | (c << 2);
      base[4 + i] = ((4u + k) << 5) | (c << 2);
      sel[i] = 0x0c020400u + (k << 8);
    }
  }
};
// XOR_k T8_{4h+k}[byte k of v]: h = 0 the r-side half of Z_8, h = 1 Z_4(v)
__device__ __forceinline__ uint32_t s_z8half(const char* lds, uint32_t v, const Z8Lane& z8, uint32_t h) {
  uint32_t y[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) y[i] = s_lds(lds, kSTab + __builtin_amdgcn_perm(v, z8.base[4 * h + i], z8.sel[i]));
  return __builtin_amdgcn_bitop3_b32(y[0], y[1], y[2], 0x96) ^ y[3];
}
// a whole unit: Z_8(v0) ^ Z_4(v1), the eight lookups folded in four ops (the
// v1 side, off the chain, first)
__device__ __forceinline__ uint32_t s_z8unit(const char* lds, uint32_t v0, uint32_t v1, const Z8Lane& z8) {
  uint32_t y[8];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) y[4 + i] = s_lds(lds, kSTab + __builtin_amdgcn_perm(v1, z8.base[4 + i], z8.sel[i]));
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) y[i] = s_lds(lds, kSTab + __builtin_amdgcn_perm(v0, z8.base[i], z8.sel[i]));
  const uint32_t t = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(y[4], y[5], y[6], 0x96), y[7], y[0], 0x96);
  return __builtin_amdgcn_bitop3_b32(t, y[1], y[2], 0x96) ^ y[3];
}

// Z_{2^m}(v), m <= 30, through the shared nibble tables in LDS (every lane
// reads table m: a nibble value picks one of 16 banks, equal values broadcast)
__device__ __forceinline__ uint32_t s_zpow2(const char* lds, uint32_t m, uint32_t v) {
  uint32_t a = 0;
  const uint32_t t = kSNib + 512u * m;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) a ^= s_lds(lds, t + 64u * i + (__builtin_amdgcn_ubfe(v, 4 * i, 4) << 2));
  return a;
}
// Z_d(v), d < 2^31, by binary powers; lanes whose d is done keep their value
__device__ __forceinline__ uint32_t s_zd(const char* lds, uint32_t d, uint32_t v) {
  for (uint32_t m = 0; __builtin_amdgcn_ballot_w64((d >> m) != 0u) != 0; ++m) {
    const uint32_t z = s_zpow2(lds, m, v);
    v = ((d >> m) & 1u) ? z : v;
  }
  return v;
}
// Z_d(v), d < 2^40 (giant frames): m > 30 from the image in HBM
__device__ __forceinline__ uint32_t s_zd64(const char* lds, const uint32_t* image, uint64_t d, uint32_t v) {
  for (uint32_t m = 0; __builtin_amdgcn_ballot_w64((d >> m) != 0u) != 0; ++m) {
    uint32_t z;
    if (m <= 30) {
      z = s_zpow2(lds, m, v);
    } else {
      const uint32_t* t = image + kStageNibHiImg + kNib8Dwords * (m - kStageNibLo);
      z = 0;
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i) z ^= t[nib8_at(0, i, __builtin_amdgcn_ubfe(v, 4 * i, 4))];
    }
    v = ((d >> m) & 1u) ? z : v;
  }
  return v;
}

// K_c = Z_{-c}(0xFFFFFFFF): (w & ~lomask(c)) ^ K_c folded by Z4 is the state,
// after the dword, of a frame that starts at its byte c
constexpr uint32_t s_unz(uint32_t v, int nbytes) {
  for (int i = 0; i < 8 * nbytes; ++i) {
    const uint32_t b = v >> 31, t = b ? v ^ 0xEDB88320u : v;
    v = (t << 1) | b;
  }
  return v;
}
constexpr uint32_t kK1 = s_unz(0xFFFFFFFFu, 1), kK2 = s_unz(0xFFFFFFFFu, 2), kK3 = s_unz(0xFFFFFFFFu, 3);

template <StageMode MODE>
__device__ __forceinline__ uint32_t stage_value(uint32_t reg, uint64_t len) {
  const uint32_t crc = ~reg;
  return MODE == StageMode::kCrc ? crc : (uint32_t)(len >= 4 && crc == 0x2144DF1Cu);
}

template <StageMode MODE>
__device__ __forceinline__ void stage_store(void* out, uint64_t f, uint32_t v) {
  if constexpr (MODE == StageMode::kCrc)
    reinterpret_cast<uint32_t*>(out)[f] = v;
  else
    reinterpret_cast<uint8_t*>(out)[f] = (uint8_t)v;
}

// ---------------------------------------------------------------- one frame, one wave
// The CRC register (init 0xFFFFFFFF) of bytes [s, e), s < e wave-uniform,
// folded by the whole wave: [B, e), B = s rounded down to a 16-byte address,
// is cut into 64 chunks of C bytes (C a multiple of 128); lane k folds the
// part of chunk k inside [s, e) from 0 (lane 0, whose part starts at s, from
// the init), 128 bytes a round, and by linearity the frame's register is
// XOR_k Z_{e - ce_k}(r_k) (ce_k = the end of lane k's part).  Each 16-byte
// load is aligned and holds a byte of [s, e) (a block past the lane's part
// re-reads the one at B), so it never leaves the frame's pages.  A round whose
// 128 bytes some lane does not own whole is folded byte by byte from the
// wave's staging area `tr` (64 x 128 bytes).  Used for the frames the staged
// blocks cannot take (out-of-order blocks, giant slices out of order).
__device__ uint32_t wave_fold(const char* lds, const uint32_t* image, const uint8_t* bytes, uint64_t s, uint64_t e,
                              char* tr, uint32_t lane, uint32_t b0, const Z8Lane& z8) {
  const uint64_t B = s - ((reinterpret_cast<uintptr_t>(bytes) + s) & 15u);
  const uint64_t C = ((e - B + 63u) / 64u + 127u) & ~127ull;
  const uint64_t c0 = B + (uint64_t)lane * C;
  const uint64_t cs = c0 > s ? c0 : s, ce = c0 + C < e ? c0 + C : e;
  const bool has = cs < ce;
  uint32_t r = lane == 0 ? 0xFFFFFFFFu : 0u;
  const uint64_t rounds = C / 128u;
  for (uint64_t t = 0; t < rounds; ++t) {
    const uint64_t p = c0 + 128u * t;
    const bool live = has && p < ce;
    u32x4 w[8];
#pragma unroll
    for (int m = 0; m < 8; ++m)
      w[m] = *reinterpret_cast<const u32x4*>(bytes + (live && p + 16u * m < ce ? p + 16u * m : B));
    const bool clean = !live || (p >= cs && p + 128u <= ce);
    if (__builtin_amdgcn_ballot_w64(!clean) == 0) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const uint32_t nr = s_z8unit(lds, r ^ w[u >> 1][(2 * u) & 3], w[u >> 1][(2 * u + 1) & 3], z8);
        r = live ? nr : r;
      }
      continue;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) *reinterpret_cast<u32x4*>(tr + 128u * lane + 16u * m) = w[m];
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = 0; i < 128u; ++i) {
      const uint64_t pos = p + i;
      const bool act = live && pos >= cs && pos < ce;
      const uint32_t byte = (uint32_t)(uint8_t)tr[128u * lane + i];
      const uint32_t nr = s_z1(lds, r ^ byte, b0);
      r = act ? nr : r;
    }
    __builtin_amdgcn_wave_barrier();
  }
  r = s_zd64(lds, image, has ? e - ce : 0u, has ? r : 0u);
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) r ^= (uint32_t)__shfl_xor((int)r, sft);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)r);
}

// ---------------------------------------------------------------- out of order
// A block whose offsets are not non-decreasing (outside the entry's contract;
// a frame whose end is below its start is empty, as in the rows kernel): one
// lane per frame up to kOooLane bytes, byte by byte, the whole wave looping to
// the longest such frame (a lane past its frame re-reads its first byte and
// keeps its register, so no load issues under narrowed exec — the audit's
// loop rule); each longer frame then by the whole wave
// (wave_fold).  Every frame gets its true CRC.
constexpr uint64_t kOooLane = 16384;
template <StageMode MODE>
__device__ __forceinline__ void ooo_block(const char* lds, const uint32_t* image, const uint8_t* bytes,
                                          const uint64_t* off, uint64_t f0, uint32_t bf, void* out, char* tr,
                                          uint32_t lane, uint32_t b0, const Z8Lane& z8) {
  for (uint32_t j0 = 0; j0 < bf; j0 += 64u) {
    const uint32_t j = j0 + lane;
    const uint64_t s = j < bf ? off[f0 + j] : 0, e0 = j < bf ? off[f0 + j + 1] : 0;
    const uint64_t len0 = e0 > s ? e0 - s : 0;
    const bool by_lane = len0 <= kOooLane;
    const uint64_t len = by_lane ? len0 : 0;
    uint32_t r = 0xFFFFFFFFu;
    for (uint64_t q = 0;; ++q) {
      const bool act = q < len;
      if (__builtin_amdgcn_ballot_w64(act) == 0) break;
      uint32_t b = 0;
      if (act) b = bytes[s + q];  // (single bytes: no multi-dword load under a narrowed exec)
      const uint32_t nr = s_z1(lds, r ^ b, b0);
      r = act ? nr : r;
    }
    if (j < bf && by_lane) stage_store<MODE>(out, f0 + j, stage_value<MODE>(r, len));
    for (uint64_t big = __builtin_amdgcn_ballot_w64(j < bf && !by_lane); big != 0; big &= big - 1u) {
      const uint32_t k = (uint32_t)__builtin_ctzll(big);
      const uint64_t fs = off[f0 + j0 + k], fe = off[f0 + j0 + k + 1];  // (every lane: one address)
      const uint32_t R = wave_fold(lds, image, bytes, fs, fe, tr, lane, b0, z8);
      if (lane == 0) stage_store<MODE>(out, f0 + j0 + k, stage_value<MODE>(R, fe - fs));
    }
  }
}

// ---------------------------------------------------------------- giant slices
// Every workgroup of the launch folds its share of the giant slices (their
// bytes do not fit 31-bit buffer offsets).  The bytes of all
// giant slices are cut into NP pieces of P bytes (P = max(16 KiB, total / 2^20
// rounded up to 16 KiB), so NP <= 2^20 + #slices); global lane t folds pieces
// t, t + T, ... (T lanes in the launch).  A lane folds its piece [a, b) as one
// byte stream in 128-byte blocks (8 dwordx4 loads, wave-uniform trip count),
// eight bytes per step through the lane-private tables; a block holding a
// frame boundary or a piece edge in some lane is folded byte by byte from LDS
// for the whole wave.  A frame inside one piece is finished there; a frame
// that crosses pieces gets, from each piece it touches, its register there
// advanced to the frame end, Z_{e - v}(r) (v = the end of its part in the
// piece), XORed into the scratch slot of the first piece boundary it crosses
// (device-scope atomics: the XOR, then a release/acquire count); the lane
// whose count completes the frame takes the XOR (leaving the slot zero for
// the next launch) and stores the result.
//
// The pieces need a slice's offsets non-decreasing (the entry's contract).
// So that a batch outside it can neither fault nor leave the scratch dirty for
// the next launch, the workgroup first checks every giant slice's offsets
// (frames numbered across the giant slices by the prefix gpre, 512 at a time);
// a slice with a decreasing pair gets no pieces, and its frames are folded
// one per wave over the whole grid instead (wave_fold; a frame whose end is
// below its start is empty, as everywhere).
template <StageMode MODE>
__device__ __forceinline__ void giant_pieces(const char* lds, const uint32_t* image, const uint8_t* bytes, const uint64_t* off,
                             uint64_t nframes, uint64_t per, uint64_t gmean, void* out, uint32_t* scratch, char* tr,
                             uint32_t* pre, uint32_t* gpre, uint32_t* badm, uint32_t lane, uint32_t b0,
                             const Z8Lane& z8) {
  const uint32_t G = gridDim.x;
  auto slice = [&](uint32_t w, uint64_t& f0, uint64_t& f1, uint64_t& s, uint64_t& span) -> bool {
    f0 = (uint64_t)w * per < nframes ? (uint64_t)w * per : nframes;
    f1 = f0 + per < nframes ? f0 + per : nframes;
    s = off[f0];
    const uint64_t e = off[f1];
    span = e > s ? e - s : 0;
    const uint64_t adj = (reinterpret_cast<uintptr_t>(bytes) + s) & 127u;
    return w < G && slice_is_giant(span, adj, f1 - f0, gmean);
  };
  // ---- the giant slices out of order (bit g of badm)
  if (threadIdx.x < 64u) {  // wave 0: gpre[w] = frames of the giant slices before w
    uint32_t carry = 0;
    for (uint32_t w0 = 0; w0 < G; w0 += 64u) {
      const uint32_t w = w0 + lane;
      uint64_t f0, f1, s, span;
      const bool gi = slice(w, f0, f1, s, span);
      const uint32_t nf = gi ? (uint32_t)(f1 - f0) : 0u;
      uint32_t inc = nf;
#pragma unroll
      for (int sft = 1; sft < 64; sft <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, sft);
        inc += lane >= (uint32_t)sft ? o : 0u;
      }
      if (w <= G) gpre[w] = carry + inc - nf;
      carry += (uint32_t)__shfl((int)inc, 63);
    }
    if (lane == 0) gpre[G] = carry;
  }
  __syncthreads();
  {
    const uint32_t TF = gpre[G];
    // four pairs a thread per step, their loads in flight together
    for (uint32_t t0 = 0; t0 < TF; t0 += 4u * kStageW * 64u) {
      uint64_t i[4];
      uint32_t g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t t = t0 + (uint32_t)u * kStageW * 64u + threadIdx.x;
        uint32_t gg = 0;
        for (uint32_t step = 256u; step > 0; step >>= 1)
          if (gg + step <= G && gpre[gg + step] <= t) gg += step;
        g[u] = gg;
        i[u] = t < TF ? (uint64_t)gg * per + (t - gpre[gg]) : 0u;  // (t past TF: pair 0, 1, never flagged below)
      }
      uint64_t a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = off[i[u]], b[u] = off[i[u] + 1];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t t = t0 + (uint32_t)u * kStageW * 64u + threadIdx.x;
        if (t < TF && b[u] < a[u])
          __hip_atomic_fetch_or(badm + (g[u] >> 5), 1u << (g[u] & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  __syncthreads();
  auto bad = [&](uint32_t w) -> bool { return w < G && ((badm[w >> 5] >> (w & 31u)) & 1u) != 0u; };
  // ---- the in-order giant slices, their total bytes and the piece prefix pre[0..G] (LDS)
  uint64_t tg = 0;
  for (uint32_t w0 = 0; w0 < G; w0 += 64u) {
    const uint32_t w = w0 + lane;
    uint64_t f0, f1, s, span;
    const bool gi = slice(w, f0, f1, s, span) && !bad(w);
    tg += gi ? span : 0;
  }
#pragma unroll
  for (int sft = 1; sft < 64; sft <<= 1) tg += (uint64_t)__shfl_xor((long long)tg, sft);
  uint64_t P = (tg + kGiantPieces - 1) / kGiantPieces;
  P = (P + kGiantPieceMin - 1) / kGiantPieceMin * kGiantPieceMin;
  P = P < kGiantPieceMin ? kGiantPieceMin : P;
  P = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)P)) |
      ((uint64_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(P >> 32)) << 32);
  uint32_t carry = 0;
  for (uint32_t w0 = 0; w0 < G; w0 += 64u) {
    const uint32_t w = w0 + lane;
    uint64_t f0, f1, s, span;
    const bool gi = slice(w, f0, f1, s, span) && !bad(w);
    const uint32_t np = gi ? (uint32_t)((span + P - 1) / P) : 0u;
    uint32_t inc = np;  // inclusive scan over the 64 lanes
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, sft);
      inc += lane >= (uint32_t)sft ? o : 0u;
    }
    if (w <= G) pre[w] = carry + inc - np;
    carry += (uint32_t)__shfl((int)inc, 63);
  }
  if (lane == 0) pre[G] = carry;
  __builtin_amdgcn_wave_barrier();
  const uint32_t NP = carry;
  const uint32_t T = G * kStageW * 64u;
  const uint32_t t0 = (blockIdx.x * kStageW + (threadIdx.x >> 6)) * 64u + lane;
  uint32_t* acc = scratch;
  uint32_t* cnt = scratch + (kGiantPieces + 4096u);
  uint32_t nsteps = 1;  // binary-search steps over a slice's per + 1 offsets
  while ((1ull << nsteps) <= per) ++nsteps;

  for (uint32_t pbase = 0; pbase < NP; pbase += T) {
    const uint32_t p = pbase + t0;
    const bool act = p < NP;
    // the lane's giant slice g: the last g with pre[g] <= p
    uint32_t g = 0;
    for (uint32_t step = 256u; step > 0; step >>= 1)
      if (g + step < G && pre[g + step] <= p) g += step;
    const uint64_t F0 = (uint64_t)g * per < nframes ? (uint64_t)g * per : nframes;
    const uint64_t F1 = F0 + per < nframes ? F0 + per : nframes;
    const uint64_t S = off[F0], E = off[F1];
    const uint64_t k = act ? p - pre[g] : 0;
    const uint64_t a = act ? S + k * P : S, b = act ? (S + (k + 1) * P < E ? S + (k + 1) * P : E) : S;
    const bool last_piece = act && b == E;
    // lb = the first frame in [F0, F1] starting at or after a (wave-uniform step count)
    uint64_t lo = F0, hi = F1;
    for (uint32_t it = 0; it < nsteps + 1u; ++it) {
      const uint64_t mid = (lo + hi) >> 1;
      const uint64_t om = off[mid];
      const bool go = lo < hi;
      lo = go && om < a ? mid + 1 : lo;
      hi = go && !(om < a) ? mid : hi;
    }
    const uint64_t lb = lo;
    const uint64_t olb = off[lb];
    // the frame the piece starts in: one that began before a, or the first at a
    const bool cross_in = lb > F0 && olb > a;
    uint64_t cur = cross_in ? lb - 1 : lb;
    uint64_t scur = cross_in ? off[lb - 1] : olb;
    uint64_t x = cur < F1 ? off[cur + 1] : ~0ull;  // the current frame's end
    // the next frame's end, loaded one advance ahead: an advance takes it and
    // issues the load of the one after, whose value is first read at the
    // lane's next advance (in the byte-serial blocks a lane's frame ends are
    // ~a frame apart; waiting for the load at every end event of every lane
    // made a 16 KiB piece of Zipf frames cost milliseconds)
    uint64_t xn = off[cur + 2u <= F1 ? cur + 2u : F1];
    uint32_t r = cross_in ? 0u : 0xFFFFFFFFu;
    // a frame's end event (its end at `at`): finish it here when all of it lies
    // in the piece, else add this piece's part
    // (every lane calls it, ev per lane).  The parts a wave's lanes add to
    // one frame (consecutive pieces of a long frame: up to 64 a wave) are
    // XORed across the wave first and added by one lane with their count, so
    // the slot of a 2 GB frame takes ~2 K atomics rather than 134 K
    // (same-address device atomics serialize at ~12 ns)
    auto frame_end = [&](bool ev, uint64_t at) {
      const bool here = scur >= a && at <= b;
      if (ev && here) stage_store<MODE>(out, cur, stage_value<MODE>(r, at - scur));
      const bool part = ev && !here;
      const uint32_t slot = part ? pre[g] + (uint32_t)((scur - S) / P) + 1u : 0u;
      for (uint64_t pend = __builtin_amdgcn_ballot_w64(part); pend != 0;) {
        const uint32_t l0 = (uint32_t)__builtin_ctzll(pend);
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)slot, (int)l0);
        const bool mine = part && slot == s0;
        const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
        uint32_t v = mine ? r : 0u;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) v ^= (uint32_t)__shfl_xor((int)v, sft);
        if (lane == l0) {
          const uint32_t np = (uint32_t)__builtin_popcountll(m);
          const uint32_t nparts = (uint32_t)((at - 1u - S) / P - (scur - S) / P + 1u);
          __hip_atomic_fetch_xor(acc + s0, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint32_t old = __hip_atomic_fetch_add(cnt + s0, np, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
          if (old + np == nparts) {
            const uint32_t tot = __hip_atomic_exchange(acc + s0, 0u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(cnt + s0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            stage_store<MODE>(out, cur, stage_value<MODE>(tot, at - scur));
          }
        }
        pend &= ~m;
      }
    };
    auto advance = [&](bool ev) {
      cur = ev ? cur + 1u : cur;
      scur = ev ? x : scur;
      r = ev ? 0xFFFFFFFFu : r;
      x = ev ? (cur < F1 ? xn : ~0ull) : x;
      xn = off[cur + 2u <= F1 ? cur + 2u : F1];  // (every lane, unconditionally: no select waits on it)
    };
    // 128-byte blocks from the line holding a
    const uint64_t blk0 = a - ((reinterpret_cast<uintptr_t>(bytes) + a) & 127u);
    uint32_t nblk = act ? (uint32_t)((b - blk0 + 127u) / 128u) : 0u;
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)nblk, sft);
      nblk = o > nblk ? o : nblk;
    }
    nblk = (uint32_t)__builtin_amdgcn_readfirstlane((int)nblk);
    for (uint32_t t = 0; t < nblk; ++t) {
      const uint64_t bp = blk0 + 128ull * t;
      const bool inb = act && bp < b;
      // (a line that holds a byte of the buffer is mapped: lanes past their
      // piece re-read the line holding a)
      const u32x4* src = reinterpret_cast<const u32x4*>(bytes + (inb ? bp : blk0));
      u32x4 w[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) w[m] = src[m];
      const bool clean = !inb || (bp >= a && bp + 128u <= b && x >= bp + 128u);
      if (__builtin_amdgcn_ballot_w64(!clean) == 0) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const uint32_t nr = s_z8unit(lds, r ^ w[u >> 1][(2 * u) & 3], w[u >> 1][(2 * u + 1) & 3], z8);
          r = inb ? nr : r;
        }
        continue;
      }
      // byte by byte, from the lane's 128 bytes staged in LDS
#pragma unroll
      for (int m = 0; m < 8; ++m) *reinterpret_cast<u32x4*>(tr + 128u * lane + 16u * m) = w[m];
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = 0; i < 128u; ++i) {
        const uint64_t pos = bp + i;
        const bool live = inb && pos >= a && pos < b;
        while (__builtin_amdgcn_ballot_w64(live && x == pos) != 0) {
          const bool ev = live && x == pos;
          frame_end(ev, pos);
          advance(ev);
        }
        const uint32_t byte = (uint32_t)(uint8_t)tr[128u * lane + i];
        const uint32_t nr = s_z1(lds, r ^ byte, b0);
        r = live ? nr : r;
      }
      __builtin_amdgcn_wave_barrier();
    }
    // the piece end b: the frame ending exactly there finishes; one that runs
    // on adds Z_{x - b}(r); the last piece also finishes the empty frames at E
    const bool endb = act && cur < F1 && x == b;
    frame_end(endb, b);
    advance(endb && last_piece);  // (frames starting at b belong to the next piece)
    while (__builtin_amdgcn_ballot_w64(last_piece && cur < F1 && x == b) != 0) {
      const bool ev = last_piece && cur < F1 && x == b;
      frame_end(ev, b);
      advance(ev);
    }
    const bool runs_on = act && !endb && cur < F1 && x > b && x != ~0ull;
    const uint32_t z = s_zd64(lds, image, runs_on ? x - b : 0u, r);
    r = runs_on ? z : r;
    frame_end(runs_on, x);
  }
  // ---- the giant slices out of order: frame i of one to wave i mod NW of the grid
  const uint32_t W = blockIdx.x * kStageW + (threadIdx.x >> 6), NW = G * kStageW;
  for (uint32_t g = 0; g < G; ++g) {
    if (!bad(g)) continue;
    const uint64_t F0 = (uint64_t)g * per < nframes ? (uint64_t)g * per : nframes;
    const uint64_t F1 = F0 + per < nframes ? F0 + per : nframes;
    for (uint64_t i = F0 + W; i < F1; i += NW) {
      const uint64_t s = off[i], e = off[i + 1];  // (every lane: one address)
      const uint32_t R = e > s ? wave_fold(lds, image, bytes, s, e, tr, lane, b0, z8) : 0xFFFFFFFFu;
      if (lane == 0) stage_store<MODE>(out, i, stage_value<MODE>(R, e > s ? e - s : 0u));
    }
  }
}

// ---------------------------------------------------------------- the kernel
template <StageMode MODE>
__global__ void __launch_bounds__(kStageW * 64, 1)
crc32_stage_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t nframes,
                   uint64_t frames_per_wg, const uint32_t* __restrict__ image, void* __restrict__ out,
                   uint32_t policy, uint32_t* __restrict__ scratch, const uint32_t* __restrict__ stage_flag,
                   uint32_t epoch) {
  // behind the rows launch (the plain entries): nothing to do unless one of
  // its workgroups found a slice for this kernel (one word, this call's epoch)
  if (stage_flag && *stage_flag != epoch) return;
  constexpr uint32_t kLast = kStageBF + 1;  // the list's last entry (a sentinel past bf)
  constexpr uint32_t kThreads = kStageW * 64;
  __shared__ __attribute__((aligned(16))) char lds[kSBytes];
  const uint64_t fb0 = (uint64_t)blockIdx.x * frames_per_wg < nframes ? (uint64_t)blockIdx.x * frames_per_wg : nframes;
  const uint64_t fb1 = fb0 + frames_per_wg < nframes ? fb0 + frames_per_wg : nframes;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  // ---- this workgroup's slice, and whether the launch has giant slices
  // (every workgroup reads the G + 1 slice bounds: L2 hits after the first)
  const uint64_t gmean = batch_mean(off, nframes);
  const uint32_t own = slice_kind(bytes, off, fb0, fb1, policy, gmean);
  bool giant = false;
  for (uint32_t w0 = 0; w0 < gridDim.x; w0 += 64u) {
    const uint32_t w = w0 + lane;
    const uint64_t f0 = (uint64_t)w * frames_per_wg < nframes ? (uint64_t)w * frames_per_wg : nframes;
    const uint64_t f1 = f0 + frames_per_wg < nframes ? f0 + frames_per_wg : nframes;
    const uint64_t s = off[f0], e = off[f1];
    const uint64_t span = e > s ? e - s : 0, adj = (reinterpret_cast<uintptr_t>(bytes) + s) & 127u;
    giant = giant || __builtin_amdgcn_ballot_w64(w < gridDim.x && slice_is_giant(span, adj, f1 - f0, gmean)) != 0;
  }
  if (own != kSliceStage && !giant) return;
  // ---- image: the T8 values expanded into their 8 bank columns, the nibble tables verbatim
  {
    const uint32_t t = threadIdx.x;
    for (uint32_t vi = t; vi < 2048u; vi += kThreads) {
      const uint32_t v = image[kStageZ8Img + vi];
      uint4* row = reinterpret_cast<uint4*>(lds + kSTab + ((vi & 255u) << 8) + ((vi >> 8) << 5));
      const uint4 v4 = {v, v, v, v};
      row[0] = v4;
      row[1] = v4;
    }
    for (uint32_t i = t; i < kStageNibLo * kNib8Dwords; i += kThreads)
      reinterpret_cast<uint32_t*>(lds + kSNib)[i] = image[kStageNibImg + i];
    if (t == 0) *reinterpret_cast<uint32_t*>(lds + kSCtr) = 0;
    if (t < 8u) reinterpret_cast<uint32_t*>(lds + kSBad)[t] = 0;
  }
  __syncthreads();
  const uint32_t b0 = (lane & 7u) << 2;
  const Z8Lane z8(lane);
  char* tr = lds + kSTr + 8192u * wv;
  uint32_t* list = reinterpret_cast<uint32_t*>(lds + kSBnd + kSList * wv);
  const uint32_t nslice = (uint32_t)(fb1 - fb0);
  constexpr uint32_t elem = MODE == StageMode::kCrc ? 4u : 1u;
  const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<char*>(out) + fb0 * elem, (short)0, (int)(nslice * elem), 0x00020000);
  // this lane's read-back addresses: piece i of its line at rb + 16 ((i + lane) & 7)
  const uint32_t rb = 1024u * (lane & 7u) + 128u * (lane >> 3), rot = lane & 7u;

  auto grab = [&]() -> uint32_t {
    uint32_t b = 0;
    if (lane == 0) b = __hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(lds + kSCtr), 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
  };

  for (;;) {
    if (own != kSliceStage) break;
    const uint32_t blk = grab();
    const uint64_t f0r = (uint64_t)blk * kStageBF;  // relative to fb0
    if (f0r >= nslice) break;
    const uint32_t bf = (uint32_t)(nslice - f0r < kStageBF ? nslice - f0r : kStageBF);
    const uint64_t f0 = fb0 + f0r;
    const uint64_t A = off[f0], E = off[f0 + bf];
    const uint8_t* pa = bytes + A;
    const uint32_t adj = (uint32_t)(reinterpret_cast<uintptr_t>(pa) & 127u);
    // ---- boundary list (relative to the line-aligned base): x_j = off[f0 + j] - A + adj;
    // a block whose offsets are out of order (an entry outside [A, E] or below
    // its predecessor) is folded one lane per frame instead
    bool ooo = E < A;
#pragma unroll
    for (uint32_t i = 0; i < (kStageBF + 2) / 64; ++i) {  // (whole-wave loads: entry j > bf re-reads entry bf)
      const uint32_t j = lane + 64u * i;
      const uint64_t o = off[f0 + (j <= bf ? j : bf)];
      ooo = ooo || o < A || o > E;
      const uint32_t x = o > A ? (uint32_t)(o - A) + adj : adj;
      list[j] = j <= bf ? x : kSNone;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t i = 0; i < (kStageBF + 2) / 64; ++i) {
      const uint32_t j = lane + 64u * i;
      ooo = ooo || (j >= 1u && j <= bf && list[j] < list[j - 1u]);
    }
    if (__builtin_amdgcn_ballot_w64(ooo) != 0) {
      ooo_block<MODE>(lds, image, bytes, off, f0, bf, out, tr, lane, b0, z8);
      __builtin_amdgcn_wave_barrier();  // the list is rewritten by the next block
      continue;
    }
    // (span < 2^31 - 2^20: the slice is not giant, dispatch.hpp)
    const uint32_t sp = (uint32_t)(E - A) + adj;
    // 64 Q > sp: the block's last boundary (at sp) must lie inside a stretch
    uint32_t Q = ((sp + 64u) / 64u + 127u) & ~127u;
    Q = Q < 128u ? 128u : Q;
    const uint32_t rounds = Q / 128u;
    // the range rounded up to whole 16-byte pieces: a load that straddles the
    // range end reads as 0, and the block's last frame ends in it (the bytes
    // past E only feed states past the last boundary; the base is 128-aligned,
    // so the piece holding E's last byte never crosses a page)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pa - adj), (short)0,
                                                                        (int)((sp + 15u) & ~15u), 0x00020000);
    // load offsets: instruction m reads stretch s = 8 (lane >> 3) + m, piece ((lane & 7) - s) & 7
    uint32_t lo_m[8];
#pragma unroll
    for (uint32_t m = 0; m < 8; ++m) {
      const uint32_t s = 8u * (lane >> 3) + m;
      lo_m[m] = s * Q + 16u * (((lane & 7u) - s) & 7u);
    }
    // Streaming loads are inline asm (hipcc neither counts them nor merges
    // their waits across the fold's branches into vmcnt(0)): every round
    // issues exactly 8 of them (rounds past the stretch get an offset past
    // the range: no memory traffic) after exactly 2 result stores, so the wait
    // for a slot is a static vmcnt(10).  The statement opens with s_nop 4 (a
    // descriptor SGPR restored by VALU needs 5 wait states before a VMEM
    // instruction reads it), outputs early-clobber.
    auto issue = [&](u32x4(&b)[8], uint32_t rr) {
      const uint32_t so = rr < rounds ? rr * 128u : kSOOB;
      asm volatile(
          "s_nop 4\n\t"
          "buffer_load_dwordx4 %0, %8, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %1, %9, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %2, %10, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %3, %11, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %4, %12, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %5, %13, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %6, %14, %16, %17 offen\n\t"
          "buffer_load_dwordx4 %7, %15, %16, %17 offen"
          : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3]), "=&v"(b[4]), "=&v"(b[5]), "=&v"(b[6]), "=&v"(b[7])
          : "v"(lo_m[0]), "v"(lo_m[1]), "v"(lo_m[2]), "v"(lo_m[3]), "v"(lo_m[4]), "v"(lo_m[5]), "v"(lo_m[6]),
            "v"(lo_m[7]), "s"(rs), "s"(so));
    };
    // results of the fast halves, held to the next round's flush (one per half)
    uint32_t hv0 = 0, hf0 = kSOOB, hv1 = 0, hf1 = kSOOB;
    auto store = [&](uint32_t v, uint32_t at) {
      if constexpr (MODE == StageMode::kCrc)
        __builtin_amdgcn_raw_buffer_store_b32(v, out_rsrc, at, 0, 0);
      else
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v, out_rsrc, at, 0, 0);
    };
    // exactly two stores per flush, in asm so that hipcc cannot merge or drop
    // them (the ring's vmcnt(10) counts them)
    auto flush = [&]() {
      if constexpr (MODE == StageMode::kCrc)
        asm volatile("buffer_store_dword %0, %1, %4, 0 offen\n\tbuffer_store_dword %2, %3, %4, 0 offen"
                     ::"v"(hv0), "v"(hf0), "v"(hv1), "v"(hf1), "s"(out_rsrc) : "memory");
      else
        asm volatile("buffer_store_byte %0, %1, %4, 0 offen\n\tbuffer_store_byte %2, %3, %4, 0 offen"
                     ::"v"(hv0), "v"(hf0), "v"(hv1), "v"(hf1), "s"(out_rsrc) : "memory");
      hf0 = hf1 = kSOOB;
    };
    // ---- this lane's stretch [Sk, Sk + Q) and its first boundary j = lower_bound(list, Sk)
    const uint32_t Sk = lane * Q;
    uint32_t lo = 0, hi = bf + 1u;
    while (__builtin_amdgcn_ballot_w64(lo < hi) != 0) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t xm = list[mid < kLast ? mid : kLast];
      if (lo < hi) {
        if (xm >= Sk) hi = mid; else lo = mid + 1u;
      }
    }
    const uint32_t jstart = lo;
    uint32_t j = lo;
    // the lane's next three boundaries: x (due), x1 (the slow-half test), x2
    // (read one advance ahead, so that an advance never waits for the list)
    uint32_t x = list[j], x1 = list[j + 1u < kLast ? j + 1u : kLast];  // (j = bf + 1 past the block end)
    uint32_t x2 = list[j + 2u < kLast ? j + 2u : kLast];
    uint32_t xprev = j > 0 ? list[j - 1u] : 0u;
    uint32_t r = 0;
    bool first = true;
    uint32_t rec_j = 0, rec_S = 0, rec_d = 0;  // the first boundary's frame (carry pending)
    bool rec = false;
    // the end of the frame at boundary j (state S, at position xe): a result,
    // or the stretch's first frame, held until the carries are known; the
    // result goes to the half's hold (slot h) or, in a byte-serial half, out at once
    auto end_at = [&](bool ev, uint32_t S, uint32_t xe, int h) {
      const bool is_first = ev && first && j > 0;
      rec_j = is_first ? j : rec_j;
      rec_S = is_first ? S : rec_S;
      rec_d = is_first ? xe - Sk : rec_d;
      rec = rec || is_first;
      const bool res = ev && !first && j > 0;
      first = ev ? false : first;
      const uint32_t crc = ~S;
      const uint32_t fr = (uint32_t)f0r + j - 1u;
      const uint32_t val = MODE == StageMode::kCrc ? crc : ((xe - xprev >= 4u && crc == 0x2144DF1Cu) ? 1u : 0u);
      const uint32_t at = res ? fr * elem : kSOOB;
      if (h == 0) {
        hv0 = res ? val : hv0, hf0 = res ? at : hf0;
      } else if (h == 1) {
        hv1 = res ? val : hv1, hf1 = res ? at : hf1;
      } else {
        store(val, at);
      }
    };
    auto advance = [&](bool ev) {
      xprev = ev ? x : xprev;
      j = ev ? j + 1u : j;
      x = ev ? x1 : x;
      x1 = ev ? x2 : x1;
      const uint32_t x3 = list[j + 2u < kLast ? j + 2u : kLast];
      x2 = ev ? x3 : x2;
    };

    // one round: wait for the slot, stage its pieces in LDS, flush the held
    // results, refill the slot two rounds ahead, fold the lane's line in two
    // 64-byte halves
    auto round_step = [&](u32x4(&cur)[8], uint32_t rr) {
      asm volatile("s_waitcnt vmcnt(10)"
                   : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3]), "+v"(cur[4]), "+v"(cur[5]),
                     "+v"(cur[6]), "+v"(cur[7]));
#pragma unroll
      for (int m = 0; m < 8; ++m) *reinterpret_cast<u32x4*>(tr + 1024 * m + 16u * lane) = cur[m];
      flush();
      issue(cur, rr + 2u);
      // the lane's whole line in one LDS round trip (both halves)
      u32x4 ql[8];
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i) ql[i] = *reinterpret_cast<const u32x4*>(tr + rb + 16u * ((i + rot) & 7u));
#pragma unroll
      for (uint32_t h = 0; h < 2; ++h) {
        const u32x4* q = ql + 4 * h;
        const uint32_t P = Sk + 128u * rr + 64u * h;
        const uint32_t rel = x - P;
        const bool in = rel < 64u;
        if (__builtin_amdgcn_ballot_w64(x1 - P < 64u) != 0) {
          // two or more boundaries in some lane's half (frames under 64
          // bytes): byte by byte, the bytes re-read from the staged line (a
          // rolled loop: this path is rare and must not bloat the fast one)
#pragma nounroll
          for (uint32_t b = 0; b < 64u; ++b) {
            const uint32_t pi = 4u * h + (b >> 4);
            const uint32_t w = s_lds(tr, rb + 16u * ((pi + rot) & 7u) + (b & 12u));
            const uint32_t pos = P + b;
            while (__builtin_amdgcn_ballot_w64(x == pos) != 0) {
              const bool ev = x == pos;
              end_at(ev, r, x, 2);
              r = ev ? 0xFFFFFFFFu : r;
              advance(ev);
            }
            r = s_z1(lds, r ^ ((w >> (8u * (b & 3u))) & 0xFFu), b0);  // (one byte: Z_1 shifts r, not w)
          }
          continue;
        }
        const uint32_t kb = in ? rel >> 2 : 99u, c = rel & 3u;
        const uint32_t lm = in ? (uint32_t)((1ull << (8u * c)) - 1ull) : 0u;
        const uint32_t Kc = c == 0u ? 0xFFFFFFFFu : c == 1u ? kK1 : c == 2u ? kK2 : kK3;
        // the boundary word patched once per half, read back from the staged
        // line: (w & ~lm) ^ K_c; the boundary unit u = kb >> 1 then enters
        // (patch, w1) for a boundary in w0 and (0, patch) for one in w1 (Z_8(0)
        // = 0 drops r), so a unit costs one compare and two selects
        const uint32_t ub = (kb >> 1) & 7u;
        const bool odd = (kb & 1u) != 0u;
        const uint2 wp = *reinterpret_cast<const uint2*>(tr + rb + 16u * ((4u * h + (ub >> 1) + rot) & 7u) +
                                                         8u * (ub & 1u));
        const uint32_t wb = __builtin_amdgcn_bitop3_b32(odd ? wp.y : wp.x, lm, Kc, 0x9A);
        const uint32_t wb0 = odd ? 0u : wb;
        const uint32_t kbu = kb >> 1;  // (49 in a lane without a boundary)
        uint32_t rc = 0;
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
          const uint32_t w0 = q[u >> 1][(2u * u) & 3u], w1 = q[u >> 1][(2u * u + 1u) & 3u];
          const bool au = kbu == u, a1 = au && odd;
          rc = au ? r : rc;
          r = s_z8unit(lds, au ? wb0 : r ^ w0, a1 ? wb : w1, z8);
        }
        const uint32_t z4t = s_z8half(lds, rc ^ wp.x, z8, 1);
        const uint32_t ecap = odd ? z4t ^ (wp.y & lm) : rc ^ (wp.x & lm);
        if (__builtin_amdgcn_ballot_w64(in) != 0) {
          // Z_c(e) = (e >> 8c) ^ XOR_{i<c} Z_{c-i}(byte i of e) = ... T8_{8-c+i}[byte i]
          uint32_t y[3];
#pragma unroll
          for (uint32_t i = 0; i < 3; ++i)
            y[i] = s_lds(lds, kSTab + __builtin_amdgcn_perm(ecap, b0, 0x0c020400u + (i << 8)) +
                                  (((8u - c + i) & 7u) << 5));
          const uint32_t sh = c == 0u ? ecap : ecap >> (8u * c);
          const uint32_t S = __builtin_amdgcn_bitop3_b32(sh, c > 0u ? y[0] : 0u, c > 1u ? y[1] : 0u, 0x96) ^
                             (c > 2u ? y[2] : 0u);
          end_at(in, S, x, (int)h);
          advance(in);
        }
      }
    };
    // the block's first two rounds, then a drain before the ring loop: hipcc
    // gives the loop's ring registers other homes than these issues' outputs
    // and copies them over in the loop preheader, which must not happen while
    // the loads are in flight (tools/prof/audit_ring.py; the round-4 build
    // happened to coalesce them).  Both rounds' loads leave back to back, so
    // waiting for the second as well costs little more than waiting for the
    // first, which round 0 does anyway.
    u32x4 buf0[8], buf1[8];
    flush();  // (two stores, so that the first waits count alike)
    issue(buf0, 0);
    flush();
    issue(buf1, 1);
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(buf0[0]), "+v"(buf0[1]), "+v"(buf0[2]), "+v"(buf0[3]), "+v"(buf0[4]), "+v"(buf0[5]),
                   "+v"(buf0[6]), "+v"(buf0[7]), "+v"(buf1[0]), "+v"(buf1[1]), "+v"(buf1[2]), "+v"(buf1[3]),
                   "+v"(buf1[4]), "+v"(buf1[5]), "+v"(buf1[6]), "+v"(buf1[7]));
    for (uint32_t rr = 0; rr < rounds; rr += 2) {
      round_step(buf0, rr);
      if (rr + 1u < rounds) round_step(buf1, rr + 1u);
      if (rr + 2u >= rounds)  // the last round: drain the ring inside the loop (the exit's copies come after it)
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(buf0[0]), "+v"(buf0[1]), "+v"(buf0[2]), "+v"(buf0[3]), "+v"(buf0[4]), "+v"(buf0[5]),
                       "+v"(buf0[6]), "+v"(buf0[7]), "+v"(buf1[0]), "+v"(buf1[1]), "+v"(buf1[2]), "+v"(buf1[3]),
                       "+v"(buf1[4]), "+v"(buf1[5]), "+v"(buf1[6]), "+v"(buf1[7]));
    }
    flush();
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(buf0[0]), "+v"(buf0[1]), "+v"(buf0[2]), "+v"(buf0[3]), "+v"(buf0[4]),
                 "+v"(buf0[5]), "+v"(buf0[6]), "+v"(buf0[7]));
    asm volatile("" : "+v"(buf1[0]), "+v"(buf1[1]), "+v"(buf1[2]), "+v"(buf1[3]), "+v"(buf1[4]), "+v"(buf1[5]),
                 "+v"(buf1[6]), "+v"(buf1[7]));
    // ---- carries: the true register at each stretch's start
    const uint32_t E1 = r;
    const bool hb = j > jstart;  // this stretch holds a boundary
    const uint32_t up = ((lane + 63u) & 63u) << 2;
    const uint32_t Ep = (uint32_t)__builtin_amdgcn_ds_bpermute((int)up, (int)E1);
    // (evaluated by every lane: under `lane == 0 || ...` hipcc runs the
    // bpermute with lane 0 masked off, and a read from an inactive lane
    // returns 0, so lane 1 saw "no boundary" in lane 0)
    const int hbv = __builtin_amdgcn_ds_bpermute((int)up, (int)hb);
    const bool hbp = (lane == 0) | (hbv != 0);
    uint32_t Pk = Ep;
    if (__builtin_amdgcn_ballot_w64(rec && !hbp) != 0) {
      // a frame longer than a stretch: P_k = Z_Q(P_{k-1}) ^ E_{k-1} through
      // stretches without a boundary (Jacobi sweeps until nothing changes)
      for (uint32_t it = 0; it < 64u; ++it) {
        const uint32_t Pp = (uint32_t)__builtin_amdgcn_ds_bpermute((int)up, (int)Pk);
        const uint32_t zq = s_zd(lds, hbp ? 0u : Q, Pp);
        const uint32_t Pn = hbp ? Ep : zq ^ Ep;
        const bool ch = Pn != Pk;
        Pk = Pn;
        if (__builtin_amdgcn_ballot_w64(ch) == 0) break;
      }
    }
    if (__builtin_amdgcn_ballot_w64(rec) != 0) {
      const uint32_t S = rec_S ^ s_zd(lds, rec ? rec_d : 0u, Pk);
      const uint32_t crc = ~S;
      const uint32_t fr = (uint32_t)f0r + rec_j - 1u;
      if constexpr (MODE == StageMode::kCrc) {
        __builtin_amdgcn_raw_buffer_store_b32(crc, out_rsrc, rec ? fr * 4u : kSOOB, 0, 0);
      } else {
        const uint32_t xa = list[rec_j > 0 ? rec_j - 1u : 0u], xe = list[rec_j];
        const uint32_t ok = (xe - xa >= 4u && crc == 0x2144DF1Cu) ? 1u : 0u;
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)ok, out_rsrc, rec ? fr : kSOOB, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();  // the list is rewritten by the next block
  }
  if (giant)
    giant_pieces<MODE>(lds, image, bytes, off, nframes, frames_per_wg, gmean, out, scratch, tr, list,
                       reinterpret_cast<uint32_t*>(lds + kSGpre), reinterpret_cast<uint32_t*>(lds + kSBad), lane, b0,
                       z8);
}

hipError_t launch_crc32_stage(const uint8_t* bytes, const uint64_t* off, uint64_t n, void* out, bool verify,
                              uint32_t policy, const void* image, uint32_t* scratch, int num_cus, hipStream_t stream,
                              const uint32_t* stage_flag, uint32_t epoch) {
  if (n == 0) return hipSuccess;
  const SlicePlan pl = slice_plan(n, num_cus);
  const uint32_t* img = static_cast<const uint32_t*>(image);
  // one workgroup per CU even when the batch has fewer slices (small n): the
  // workgroups past the last slice own nothing and exit after the prologue,
  // unless the launch has giant slices, whose pieces every workgroup folds
  const unsigned grid = (unsigned)(pl.grid > (uint64_t)num_cus ? pl.grid : (uint64_t)num_cus);
  if (verify)
    hipLaunchKernelGGL(crc32_stage_kernel<StageMode::kVerify>, dim3(grid), dim3(kStageW * 64), 0, stream, bytes, off,
                       n, pl.per, img, out, policy, scratch, stage_flag, epoch);
  else
    hipLaunchKernelGGL(crc32_stage_kernel<StageMode::kCrc>, dim3(grid), dim3(kStageW * 64), 0, stream, bytes, off, n,
                       pl.per, img, out, policy, scratch, stage_flag, epoch);
  return hipGetLastError();
}

}  // namespace lnx
