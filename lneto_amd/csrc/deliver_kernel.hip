// deliver_kernel.hip — receive delivery on gfx950: for every
// frame the handler lneto's receive path hands it to once the verdict is in
// (deliver_plan.hpp: EtherType, IP protocol, StackPorts.Demux's port stage,
// internet/stack-ports.go:64-84), as one 16-byte lnx_rx_delivery record, and
// the frames grouped by handler in arrival order.
//
// Four launches on the caller's stream, none of which waits for another
// workgroup (no look-back, no grid barrier, no spin; the launches' order on the
// stream is the only dependency):
//   records   one 16-lane row per frame, header bytes only;
// then the slice walk of slice_walk.hpp, a count per bucket:
//   histogram each workgroup counts the buckets of ONE contiguous index slice;
//   scan      per bucket, over the workgroups in index order;
//   scatter   each workgroup walks its slice again in index order.
// The counts use LDS atomics only (their order cannot change a count); every
// position of d_order is a pure function of the keys.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "deliver_plan.hpp"
#include "launch.hpp"
#include "rx_filter.hpp"
#include "slice_walk.hpp"

namespace lnxd {

constexpr int kRecBlock = 256;                 // 16 rows: 16 frames a pass
constexpr uint32_t kRecRows = kRecBlock / 16;
constexpr uint32_t kRecGridCap = 2048;         // workgroups of the records launch (grid-strided past it)
// the header window of a row: 32 aligned dwords from the one holding the
// frame's first byte.  The rules read frame offsets below 14 + 60 + 14 = 88,
// at most 3 bytes into the window's first dword: 91 <= 128.
constexpr uint32_t kWinDwords = 32, kWinBytes = 4 * kWinDwords, kWinFrame = kWinBytes - 3;

// (kGrpBlock, kGrpGridCap and kScanWaves are restated in tests/test_deliver_gpu.py and tests/test_deliver_grid_mid.py)
constexpr int kGrpBlock = 256;                 // frames per chunk: one per thread (tests: CHUNK)
constexpr uint32_t kGrpGridCap = 512;          // workgroups of the histogram / scatter launches (tests: GRID_CAP)
constexpr uint32_t kBuckets = kHCount + 1;     // handler ids, then the frames not delivered
constexpr uint32_t kDeadKey = 2047;            // 11 key bits; no frame has it
static_assert(kBuckets <= kDeadKey && kBuckets <= 5 * kGrpBlock, "bucket keys: 11 bits, five per thread in the scan");

// ------------------------------------------------------------------ records
// frame f = bytes[off[f] : off[f + 1]], its last `trim` bytes the FCS.  A row
// (16 lanes) takes one frame: lane rl loads the window's dwords rl and rl + 16
// when they hold a byte of the frame's first L bytes (nothing else is loaded:
// the record of a frame depends on its own bytes only, and a dword that holds
// one of them lies in that byte's page), the row stages them in LDS, and every
// lane of the row reads the fields there and takes the same decisions.  The
// port search is the row's: lane rl compares entries rl, rl + 16, ... and the
// row takes the least matching index (nodeByPort's first match).  Lane 0 of the
// row stores the record, and the bucket key for the grouping launches.
__global__ void __launch_bounds__(kRecBlock)
deliver_records_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, uint64_t n, uint32_t trim,
                       lnx::RxFilter filt, DlvPorts ports, const uint8_t* __restrict__ fcs_ok,
                       const uint8_t* __restrict__ verdict, uint4* __restrict__ rec, uint16_t* __restrict__ keys) {
  __shared__ uint16_t tab[2 * kPortsMax];  // tcp, then udp
  __shared__ __attribute__((aligned(16))) uint32_t win[kRecRows * kWinDwords];
  const uint32_t t = threadIdx.x, rl = t & 15u, row = t >> 4;
  for (uint32_t i = t; i < 2 * kPortsMax; i += kRecBlock)
    tab[i] = i < kPortsMax ? ports.tcp[i] : ports.udp[i - kPortsMax];
  const uint32_t nt = ports.n_tcp < kPortsMax ? ports.n_tcp : kPortsMax;
  const uint32_t nu = ports.n_udp < kPortsMax ? ports.n_udp : kPortsMax;
  const uint32_t steps = ((nt > nu ? nt : nu) + 15u) >> 4;  // (uniform: the search's trip count)
  const uint8_t* wb = reinterpret_cast<const uint8_t*>(win) + row * kWinBytes;
  for (uint64_t g = (uint64_t)blockIdx.x * kRecRows; g < n; g += (uint64_t)gridDim.x * kRecRows) {
    const uint64_t f = g + row;
    const bool valid = f < n;
    const uint64_t s = valid ? off[f] : 0, e = valid ? off[f + 1] : 0;
    const uint32_t L = lnx::frame_len(s, e, trim);
    const uint8_t* p = bytes + s;
    const uint32_t q = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t ndw = L == 0 ? 0u : (q + (L < kWinFrame ? L : kWinFrame) + 3u) >> 2;  // <= kWinDwords
    __syncthreads();  // the last pass's reads of win (and, first, the tables' stores)
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t d = rl + 16u * k;
      uint32_t w = 0;
      if (d < ndw) w = *reinterpret_cast<const uint32_t*>(p - q + 4u * d);
      win[row * kWinDwords + d] = w;
    }
    __syncthreads();
    const uint32_t v_in = valid ? verdict[f] : 0u;
    const int32_t fcs = fcs_ok ? (valid ? (int32_t)(fcs_ok[f] != 0) : 1) : -1;
    // (a field the rules read lies below L and below 88: inside the window)
    auto byt = [&](uint32_t o) -> uint32_t { return wb[(q + o) & (kWinBytes - 1u)]; };
    auto be16 = [&](uint32_t o) -> uint32_t { return (byt(o) << 8) | byt(o + 1u); };
    DlvPlan r = dlv_parse(L, v_in, fcs, filt, be16, byt);
    int32_t k = (int32_t)kPortsMax;
    if (ports.on) {
      const uint32_t base = r.lookup == 6 ? 0u : kPortsMax;
      const uint32_t cnt = r.lookup == 6 ? nt : r.lookup == 17 ? nu : 0u;
      uint32_t best = 0xFFFFu;
      for (uint32_t j = 0; j < steps; ++j) {
        const uint32_t i = 16u * j + rl;
        if (i < cnt && tab[base + i] == r.dst_port) best = min(best, i);
      }
      best = lnx::row_min16(best);
      k = best == 0xFFFFu ? -1 : (int32_t)best;
    }
    dlv_finish(r, k);
    if (valid && rl == 0) {
      uint32_t w[4];
      dlv_pack(r, w);
      rec[f] = uint4{w[0], w[1], w[2], w[3]};
      if (keys) keys[f] = (uint16_t)dlv_bucket(r);
    }
  }
}

// ------------------------------------------------------------------ grouping
// The histogram and the scatter launch walk the same slices (slice_walk.hpp slice_bounds).
__device__ __forceinline__ uint32_t grp_key(const uint16_t* keys, uint64_t i) {
  const uint32_t k = keys[i];
  return k < kBuckets ? k : kBuckets - 1u;  // (the records launch writes nothing larger)
}

// hist[g][b] = the frames of workgroup g's slice in bucket b
__global__ void __launch_bounds__(kGrpBlock)
deliver_hist_kernel(const uint16_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kBuckets];
  for (uint32_t b = threadIdx.x; b < kBuckets; b += kGrpBlock) h[b] = 0;
  __syncthreads();
  uint64_t lo, hi;
  lnx::slice_bounds(n, kGrpBlock, lo, hi);
  for (uint64_t i = lo + threadIdx.x; i < hi; i += kGrpBlock) atomicAdd(&h[grp_key(keys, i)], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kBuckets; b += kGrpBlock) hist[(uint64_t)blockIdx.x * kBuckets + b] = h[b];
}

// hist[g][b] becomes the bucket's frames in the workgroups before g, count[b]
// the bucket's size.  A workgroup takes 64 buckets (one a lane); its wave w
// takes the workgroups [w seg, (w + 1) seg) of the histogram launch: all its
// loads at once, the waves' totals joined through LDS.
constexpr uint32_t kScanWaves = 16, kScanSeg = 32;  // kScanWaves: SCAN_WAVES in tests/test_deliver_grid_mid.py
static_assert(kGrpGridCap <= kScanWaves * kScanSeg, "the scan holds a wave's segment in registers");
__global__ void __launch_bounds__(64 * kScanWaves)
deliver_scan_kernel(uint32_t* __restrict__ hist, uint32_t G, uint32_t* __restrict__ count) {
  __shared__ uint32_t tot[kScanWaves][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t b = blockIdx.x * 64u + lane;
  const uint32_t seg = (G + kScanWaves - 1u) / kScanWaves;  // <= kScanSeg
  const uint32_t g0 = wave * seg;
  uint32_t c[kScanSeg], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanSeg; ++j) {
    const bool in = j < seg && g0 + j < G && b < kBuckets;
    c[j] = in ? hist[(uint64_t)(g0 + j) * kBuckets + b] : 0u;
    sum += c[j];
  }
  tot[wave][lane] = sum;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t w = 0; w < wave; ++w) run += tot[w][lane];
#pragma unroll
  for (uint32_t j = 0; j < kScanSeg; ++j) {
    if (j < seg && g0 + j < G && b < kBuckets) hist[(uint64_t)(g0 + j) * kBuckets + b] = run;
    run += c[j];
  }
  if (wave == kScanWaves - 1u && b < kBuckets) count[b] = run;
}

// order[position] = frame index.  run[b] starts at the bucket's base (the sizes
// of the buckets below it) plus its frames in the workgroups before this one,
// and advances as the workgroup walks its slice in index order: a chunk of
// kGrpBlock frames at a time, and within the chunk wave by wave; within the
// wave a frame's rank among the lanes of its bucket is the count of those
// below it (the lanes with an equal key from eleven ballots).
__global__ void __launch_bounds__(kGrpBlock)
deliver_scatter_kernel(const uint16_t* __restrict__ keys, uint64_t n, const uint32_t* __restrict__ hist,
                       const uint32_t* __restrict__ count, uint32_t* __restrict__ order) {
  __shared__ uint32_t run[kBuckets];
  __shared__ uint32_t part[kGrpBlock];
  const uint32_t t = threadIdx.x, wave = t >> 6;
  {
    // exclusive scan of count: thread t holds buckets 5 t .. 5 t + 4
    uint32_t c[5], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) {
      const uint32_t b = 5u * t + j;
      c[j] = b < kBuckets ? count[b] : 0u;
      sum += c[j];
    }
    uint32_t base = lnx::block_scan_inclusive<kGrpBlock>(part, sum) - sum;
#pragma unroll
    for (uint32_t j = 0; j < 5; ++j) {
      const uint32_t b = 5u * t + j;
      if (b < kBuckets) run[b] = base + hist[(uint64_t)blockIdx.x * kBuckets + b];
      base += c[j];
    }
    __syncthreads();
  }
  uint64_t lo, hi;
  lnx::slice_bounds(n, kGrpBlock, lo, hi);
  for (uint64_t c0 = lo; c0 < hi; c0 += kGrpBlock) {  // (uniform: every wave keeps all its lanes)
    const uint64_t i = c0 + t;
    const bool live = i < hi;
    const uint32_t key = live ? grp_key(keys, i) : kDeadKey;
    uint64_t same = ~0ull;
#pragma unroll
    for (uint32_t bit = 0; bit < 11; ++bit) {
      const bool one = (key >> bit) & 1u;
      const uint64_t m = __builtin_amdgcn_ballot_w64(one);
      same &= one ? m : ~m;
    }
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
    const uint32_t cnt = (uint32_t)__builtin_popcountll(same);
    const uint32_t first = (uint32_t)__builtin_ctzll(same);  // the bucket's lowest lane in this wave (same holds the lane itself)
    uint32_t pos = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < (uint32_t)kGrpBlock / 64u; ++w) {
      if (wave == w) {  // (the whole wave)
        // one lane per bucket touches run[]: it takes the bucket's lanes' places at once and hands the start to them
        uint32_t r0 = 0;
        if (live && below == 0) r0 = atomicAdd(&run[key], cnt);
        pos = (uint32_t)__shfl((int)r0, (int)first) + below;
      }
      __syncthreads();
    }
    if (live && pos < n) order[pos] = (uint32_t)i;
  }
}

// ws: the workgroups' histograms (G x kBuckets words), then the frames' keys
static uint32_t grp_workgroups(uint64_t n) { return lnx::slice_grid(n, kGrpBlock, kGrpGridCap); }
uint64_t deliver_ws_bytes(uint64_t n) { return (uint64_t)grp_workgroups(n) * kBuckets * 4u + 2u * n; }

// the keys' place in ws (n: the frames the grouping launches will take)
uint16_t* deliver_keys(void* ws, uint64_t n) {
  return reinterpret_cast<uint16_t*>(static_cast<uint32_t*>(ws) + (uint64_t)grp_workgroups(n) * kBuckets);
}

// The three grouping launches over keys that launches before them on `stream`
// wrote at deliver_keys(ws, n): the records launch below, or the receive check
// that writes records and keys itself (rx_verify_kernel.hip).
hipError_t launch_deliver_group(uint64_t n, uint32_t* order, uint32_t* count, void* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t G = grp_workgroups(n);
  uint32_t* hist = static_cast<uint32_t*>(ws);
  const uint16_t* keys = deliver_keys(ws, n);
  hipError_t e;
  hipLaunchKernelGGL(deliver_hist_kernel, dim3(G), dim3(kGrpBlock), 0, stream, keys, n, hist);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(deliver_scan_kernel, dim3((kBuckets + 63u) / 64u), dim3(64 * kScanWaves), 0, stream, hist, G,
                     count);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(deliver_scatter_kernel, dim3(G), dim3(kGrpBlock), 0, stream, keys, n, hist, count, order);
  return hipGetLastError();
}

// ports NULL: no tables.  order / count both NULL: the records alone.
hipError_t launch_deliver(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx::RxFilter& filt,
                          const lnx_rx_ports* ports, const uint8_t* fcs_ok, const uint8_t* verdict, lnx_rx_delivery* rec,
                          uint32_t* order, uint32_t* count, void* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const DlvPorts pt = dlv_ports_of(ports);
  uint16_t* keys = order ? deliver_keys(ws, n) : nullptr;
  uint64_t grid = (n + kRecRows - 1) / kRecRows;
  if (grid > kRecGridCap) grid = kRecGridCap;
  hipLaunchKernelGGL(deliver_records_kernel, dim3((unsigned)grid), dim3(kRecBlock), 0, stream, bytes, off, n, trim, filt,
                     pt, fcs_ok, verdict, reinterpret_cast<uint4*>(rec), keys);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !order) return e;
  return launch_deliver_group(n, order, count, ws, stream);
}

}  // namespace lnxd
