// api.cpp — C-ABI of the batched HIP path: per-device context (the table
// images of table_images.cpp in device memory), argument checks, host-memory
// and multi-GPU conveniences.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/lneto_amd.h"
#include "dispatch.hpp"
#include "launch.hpp"
#include "rx_filter.hpp"
#include "table_images.hpp"

namespace lnx {

namespace {

thread_local std::string g_last_error;

int hip_fail(hipError_t e, const char* what) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return LNX_EHIP;
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// The n == 0 path of the entries that report counts: `words` zero words at p, when the caller gave a p.
int zero_words(uint32_t* p, uint32_t words, hipStream_t hs, const char* what) {
  if (!p) return LNX_OK;
  const hipError_t e = hipMemsetAsync(p, 0, words * sizeof(uint32_t), hs);
  return e == hipSuccess ? LNX_OK : hip_fail(e, what);
}

// What the two delivery entries refuse alike (`allowed`: the entry's flag bits).
bool deliver_args_ok(const lnx_rx_filter* filter, RxFilter* filt, uint32_t flags, uint32_t allowed, const lnx_rx_ports* ports,
                     uint64_t n, const lnx_rx_delivery* d_rec, const uint32_t* d_order, const uint32_t* d_count,
                     const void* d_ws) {
  if (!rx_filter_of(filter, filt)) return false;
  if (flags & ~allowed) return false;
  if (ports && (ports->n_tcp > 256u || ports->n_udp > 256u)) return false;
  if ((d_order == nullptr) != (d_count == nullptr)) return false;
  if (n >> 32) return false;
  return !(misaligned(d_rec, 16) || misaligned(d_order, 4) || misaligned(d_count, 4) || misaligned(d_ws, 4));
}

// What the two record-driven reply entries refuse alike (ws_align: of the entry's workspace).
bool reply_args_ok(uint32_t flags, const lnx_rst_cfg* cfg, uint64_t n, const uint8_t* d_reply, const lnx_rx_delivery* d_rec,
                   const uint32_t* d_src, const uint32_t* d_n, const void* d_ws, uintptr_t ws_align, const uint16_t* d_ip_id) {
  if (flags & ~(uint32_t)LNX_RX_NO_FCS) return false;
  if (cfg && (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return false;
  if (n >> 32) return false;
  return !(misaligned(d_reply, 64) || misaligned(d_rec, 16) || misaligned(d_src, 4) || misaligned(d_n, 4) ||
           misaligned(d_ws, ws_align) || misaligned(d_ip_id, 2));
}

struct DeviceCtx {
  std::mutex mu;                   // serializes initialization
  std::atomic<bool> ready{false};  // set once every field below is valid
  void* d_image = nullptr;
  int num_cus = 0;
  uint32_t* d_search = nullptr;  // crc32_search_kernel tables
  uint32_t* d_stage = nullptr;   // crc32_stage_kernel image
  uint32_t* d_rx = nullptr;      // rx_verify_kernel image
  uint32_t* d_rst = nullptr;     // rst_reply_kernel image
  uint32_t* d_echo = nullptr;    // echo_reply_kernel image
  // Per stream: the staged kernel's giant-slice slots (stage_kernel.hip
  // giant_pieces; zero between launches) and the gate words of the two-launch
  // entries.  Launches on one stream run in order, so each stream owns one
  // set; streams never share one.  hipStreamPerThread names a different stream
  // in every thread, so it is keyed by thread too.  At most kGiantStreams sets
  // live per device; the least recently used one that no call holds is freed
  // (after a device sync) to make room.
  //
  // Who holds what: giant_mu guards the list, the clock and
  // every set's pins, and is held only while a call looks its set up or makes
  // one.  A call then takes its set's own mutex, draws its epoch under it and
  // keeps it until its last launch that uses the epoch is enqueued
  // (ScratchHold), so the launches of one call reach the stream as a unit with
  // respect to every other call on that set.  The sets are heap objects: their
  // addresses outlive the list's reallocations, and a set with pins > 0 is
  // never evicted.
  struct GiantScratch {
    hipStream_t stream;
    std::thread::id thread;
    uint32_t* p;
    uint64_t used = 0;          // use counter at the last call (under giant_mu)
    std::atomic<int> pins{0};   // calls between lookup and release (raised under giant_mu)
    std::mutex mu;              // held while a call enqueues its launches
    uint32_t epoch = 0;         // the last call's epoch (under mu): the gate words' value
  };
  std::mutex giant_mu;
  std::vector<std::unique_ptr<GiantScratch>> giant;
  uint64_t giant_clock = 0;
#ifdef LNX_RESEARCH
  // Per-stream scratch of the two-launch TX append (the CRCs between its
  // launches): calls on one stream run in order, so each stream reuses its
  // buffer; it grows, after a sync of that stream, when a batch outgrows it.
  struct Scratch {
    hipStream_t stream;
    void* p;
    size_t cap;
  };
  std::mutex scratch_mu;
  std::vector<Scratch> scratch;
#endif
};

constexpr int kMaxDevices = 64;
DeviceCtx g_ctx[kMaxDevices];

// Context of the calling thread's current device (created on first use).  A
// failed initialization (e.g. hipMalloc out of memory) frees what it had
// allocated and leaves the context uninitialized, so a later call retries.
int init_ctx(DeviceCtx& c, int dev) {
  auto fail = [&](hipError_t err, const char* what) {
    (void)hipFree(c.d_image);
    (void)hipFree(c.d_search);
    (void)hipFree(c.d_stage);
    (void)hipFree(c.d_rx);
    (void)hipFree(c.d_rst);
    (void)hipFree(c.d_echo);
    c.d_image = nullptr;
    c.d_search = nullptr;
    c.d_stage = nullptr;
    c.d_rx = nullptr;
    c.d_rst = nullptr;
    c.d_echo = nullptr;
    return hip_fail(err, what);
  };
  const hipError_t err = hipDeviceGetAttribute(&c.num_cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (err != hipSuccess) return fail(err, "hipDeviceGetAttribute");
  // one table image into device memory of its own
  auto upload = [&](auto** dst, const std::vector<uint32_t>& img, const std::string& name) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), img.size() * 4);
    if (e != hipSuccess) return fail(e, ("hipMalloc(" + name + ")").c_str());
    e = hipMemcpy(*dst, img.data(), img.size() * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? LNX_OK : fail(e, ("hipMemcpy(" + name + ")").c_str());
  };
  int st = upload(&c.d_image, host_image(), "image");
  if (st == LNX_OK) st = upload(&c.d_search, build_search_tables(), "search tables");
  if (st == LNX_OK) st = upload(&c.d_stage, build_stage_image(), "stage image");
  if (st == LNX_OK) st = upload(&c.d_rx, build_rx_image(), "rx image");
  if (st == LNX_OK) st = upload(&c.d_rst, build_rst_image(), "rst image");
  if (st == LNX_OK) st = upload(&c.d_echo, build_echo_image(), "echo image");
  return st;
}

int get_ctx(DeviceCtx** out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
  if (dev < 0 || dev >= kMaxDevices) return LNX_ENODEV;
  DeviceCtx& c = g_ctx[dev];
  if (!c.ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(c.mu);
    if (!c.ready.load(std::memory_order_relaxed)) {
      const int st = init_ctx(c, dev);
      if (st != LNX_OK) return st;
      c.ready.store(true, std::memory_order_release);
    }
  }
  *out = &c;
  return LNX_OK;
}

// Slots of the giant slices: acc[kGiantSlots] then cnt[kGiantSlots]
// (stage_kernel.hip: at most 2^20 pieces plus one per slice), then the flag
// word through which the rows launch tells the staged launch it has work
// (the call's epoch: nonzero, new every call on the stream, so the word needs
// no reset)
constexpr size_t kGiantSlots = (1u << 20) + 4096u;
constexpr size_t kStageFlag = 2 * kGiantSlots;
constexpr size_t kIngressGate = kStageFlag + 1;  // lnx_ingress_verify_batch's second launch (the same epoch rule)
constexpr size_t kTxChecksumGate = kStageFlag + 2;  // lnx_tx_checksum_batch's
constexpr size_t kScratchWords = kStageFlag + 16;
// the mean frame length from which the ingress rows beat the receive check
// without its CRC (tools/prof/ingress_vs_rv.py)
constexpr uint64_t kIngressShortMean = 1280;
// ... and the generate rows against tx_finish's checksum step (sampled mean)
constexpr uint64_t kTxChecksumShortMean = 896;

// A call's hold on its stream's scratch set: the set's mutex, from the epoch
// until the call's last gated launch is enqueued.  Releasing it unlocks the
// set and lets it be evicted again.
struct ScratchHold {
  DeviceCtx::GiantScratch* g = nullptr;
  uint32_t* p = nullptr;
  uint32_t epoch = 0;
  ScratchHold() = default;
  ScratchHold(const ScratchHold&) = delete;
  ScratchHold& operator=(const ScratchHold&) = delete;
  ~ScratchHold() {
    if (!g) return;
    g->mu.unlock();
    g->pins.fetch_sub(1, std::memory_order_release);
  }
};

// The calling device's giant-slice scratch for `stream`, zeroed on that
// stream when made (stream order puts the zeroing before the first launch),
// locked for the caller with a new epoch (nonzero, new every call on the set).
// The wait for the set's mutex is for another thread's enqueue on the same
// stream only, and happens outside giant_mu: calls on other streams go on.
constexpr size_t kGiantStreams = 32;
int giant_scratch(DeviceCtx* c, hipStream_t stream, ScratchHold* hold) {
  const std::thread::id tid = stream == hipStreamPerThread ? std::this_thread::get_id() : std::thread::id();
  DeviceCtx::GiantScratch* g = nullptr;
  while (!g) {
    std::unique_lock<std::mutex> lk(c->giant_mu);
    ++c->giant_clock;
    for (auto& x : c->giant)
      if (x->stream == stream && x->thread == tid) g = x.get();
    if (!g) {
      hipError_t e;
      if (c->giant.size() >= kGiantStreams) {
        // the least recently used set that no call holds; its stream may still
        // run a launch on it (or be gone): wait for the device
        auto lru = c->giant.end();
        for (auto it = c->giant.begin(); it != c->giant.end(); ++it)
          if ((*it)->pins.load(std::memory_order_acquire) == 0 && (lru == c->giant.end() || (*it)->used < (*lru)->used))
            lru = it;
        if (lru == c->giant.end()) {  // every set is mid-call (kGiantStreams threads at once): let one finish
          lk.unlock();
          std::this_thread::yield();
          continue;
        }
        if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "hipDeviceSynchronize(giant-slice scratch)");
        (void)hipFree((*lru)->p);
        c->giant.erase(lru);
      }
      uint32_t* p = nullptr;
      e = hipMalloc(reinterpret_cast<void**>(&p), kScratchWords * sizeof(uint32_t));
      if (e != hipSuccess) return hip_fail(e, "hipMalloc(giant-slice scratch)");
      if ((e = hipMemsetAsync(p, 0, kScratchWords * sizeof(uint32_t), stream)) != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "hipMemsetAsync(giant-slice scratch)");
      }
      c->giant.push_back(std::make_unique<DeviceCtx::GiantScratch>());
      g = c->giant.back().get();
      g->stream = stream, g->thread = tid, g->p = p;
    }
    g->used = c->giant_clock;
    g->pins.fetch_add(1, std::memory_order_relaxed);
  }
  g->mu.lock();
  g->epoch = g->epoch + 1u == 0u ? 1u : g->epoch + 1u;
  hold->g = g;
  hold->p = g->p;
  hold->epoch = g->epoch;
  return LNX_OK;
}

// CRC-32 / FCS verify of an offsets batch: the rows kernel,
// then the staged kernel, over the same slices; each workgroup folds its slice
// only if dispatch.hpp's slice_kind() gives it to its kernel, and the staged
// launch folds the giant slices.  policy kPolicyShort (LNX_BATCH_SHORT_FRAMES)
// gives every slice that fits to the staged kernel, so the rows launch is
// skipped.  The plain and _ex entries below are its only callers.
int crc_offsets(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, void* d_out, bool verify, uint32_t policy,
                hipStream_t stream) {
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  ScratchHold hold;  // until both launches are enqueued
  if ((st = giant_scratch(c, stream, &hold)) != LNX_OK) return st;
  uint32_t* const scratch = hold.p;
  const uint32_t epoch = hold.epoch;
  hipError_t e = hipSuccess;
  // auto: the rows launch stores the epoch in the flag word when a slice is
  // not its own, and the staged launch behind it exits at once otherwise
  uint32_t* flag = policy == kPolicyAuto ? scratch + kStageFlag : nullptr;
  if (policy == kPolicyAuto)
    e = launch_crc32_frames(d_bytes, d_off, n, d_out, verify, c->d_image, c->num_cus, stream, policy, flag, epoch);
  if (e != hipSuccess) return hip_fail(e, "crc32_rows_kernel launch");
  e = launch_crc32_stage(d_bytes, d_off, n, d_out, verify, policy, c->d_stage, scratch, c->num_cus, stream, flag,
                         epoch);
  if (e != hipSuccess) return hip_fail(e, "crc32_stage_kernel launch");
  return LNX_OK;
}

int crc_common(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, void* d_out, bool verify,
               uint32_t flags, void* stream) {
  if (flags & ~LNX_BATCH_SHORT_FRAMES) return LNX_EINVAL;
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_out) return LNX_EINVAL;
  return crc_offsets(d_bytes, d_off, n, d_out, verify, (flags & LNX_BATCH_SHORT_FRAMES) ? kPolicyShort : kPolicyAuto,
                     static_cast<hipStream_t>(stream));
}
}  // namespace

// For rx_ring.hip (launch.hpp): the current device's images and CU count, and
// the thread's lnx_last_error.
int device_resources(const void** image, int* num_cus, const void** stage_image, const void** rx_image) {
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  *image = c->d_image;
  *num_cus = c->num_cus;
  if (stage_image) *stage_image = c->d_stage;
  if (rx_image) *rx_image = c->d_rx;
  return LNX_OK;
}
int hip_error(hipError_t e, const char* what) { return hip_fail(e, what); }

}  // namespace lnx

using namespace lnx;

extern "C" {

int lnx_crc32_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t* d_crc,
                    void* stream) {
  return crc_common(d_bytes, d_off, n, d_crc, false, 0, stream);
}

int lnx_fcs_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint8_t* d_ok,
                         void* stream) {
  return crc_common(d_bytes, d_off, n, d_ok, true, 0, stream);
}

int lnx_crc32_batch_ex(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t* d_crc, uint32_t flags,
                       void* stream) {
  return crc_common(d_bytes, d_off, n, d_crc, false, flags, stream);
}

int lnx_fcs_verify_batch_ex(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint8_t* d_ok,
                            uint32_t flags, void* stream) {
  return crc_common(d_bytes, d_off, n, d_ok, true, flags, stream);
}

int lnx_sum16_batch(const uint8_t* d_bytes, const uint64_t* d_off, const uint32_t* d_len,
                    const uint32_t* d_seed, uint64_t n, uint16_t* d_out, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_len || !d_out) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  hipError_t e = launch_sum16_segments(d_bytes, d_off, d_len, d_seed, n, d_out, c->num_cus,
                                       static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "sum16_segments_kernel launch");
  return LNX_OK;
}

#ifdef LNX_RESEARCH
// The calling device's scratch for `stream`, at least `bytes` long.  The
// caller holds c->scratch_mu until its launches on the scratch are enqueued,
// so a concurrent grow (which syncs the stream, then frees) cannot free it
// under a launch that is not yet in the stream.
static int stream_scratch(DeviceCtx* c, hipStream_t stream, size_t bytes, void** out) {
  DeviceCtx::Scratch* sc = nullptr;
  for (auto& x : c->scratch)
    if (x.stream == stream) sc = &x;
  if (!sc) {
    c->scratch.push_back({stream, nullptr, 0});
    sc = &c->scratch.back();
  }
  if (sc->cap < bytes) {
    hipError_t e;
    if (sc->p) {  // the stream's earlier launches may still read the old buffer
      if ((e = hipStreamSynchronize(stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize(scratch)");
      (void)hipFree(sc->p);
      sc->p = nullptr, sc->cap = 0;
    }
    const size_t want = bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 4;
    if ((e = hipMalloc(&sc->p, want)) != hipSuccess) return hip_fail(e, "hipMalloc(scratch)");
    sc->cap = want;
  }
  *out = sc->p;
  return LNX_OK;
}
#endif  // LNX_RESEARCH

int lnx_crc32_segments(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t n,
                       uint32_t* d_crc, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_start || !d_len || !d_crc) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  hipError_t e = launch_crc32_segments(d_bytes, d_start, d_len, n, d_crc, c->d_image, c->num_cus,
                                       static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "crc32_rows_kernel (segments) launch");
  return LNX_OK;
}

int lnx_crc32_combine_batch(const uint32_t* d_crc_a, const uint32_t* d_crc_b, const uint64_t* d_len_b, uint64_t n,
                            uint32_t* d_out, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_crc_a || !d_crc_b || !d_len_b || !d_out) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxc::launch_combine_pairs(d_crc_a, d_crc_b, d_len_b, n, d_out, c->num_cus,
                                                  static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "combine_pairs_kernel launch");
  return LNX_OK;
}

int lnx_crc32_update_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, const uint32_t* d_seed,
                           uint32_t* d_crc, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_crc) return LNX_EINVAL;
  if (d_seed) {
    // the second launch reads seed[i] after the first wrote crc[i]: the arrays must be disjoint
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_seed), b = reinterpret_cast<uintptr_t>(d_crc);
    const uintptr_t bytes = (uintptr_t)n * sizeof(uint32_t);
    if (a < b + bytes && b < a + bytes) return LNX_EINVAL;
  }
  // lnx_crc32_batch's launches into d_crc, then d_crc[i] ^= Z_{len_i}(d_seed[i]) behind them on the stream
  int st = crc_common(d_bytes, d_off, n, d_crc, false, 0, stream);
  if (st != LNX_OK || !d_seed) return st;
  DeviceCtx* c = nullptr;
  if ((st = get_ctx(&c)) != LNX_OK) return st;
  const hipError_t e = lnxc::launch_seed_pairs(d_seed, d_off, n, d_crc, c->num_cus, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "combine_pairs_kernel (seed) launch");
  return LNX_OK;
}

// lnx_crc32_chain_batch / lnx_fcs_verify_chain_batch: lnx_crc32_segments' launch into the caller's d_seg_crc,
// then the fold of each frame's (CRC, length) pairs.
static int chain_common(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                        const uint64_t* d_first, uint64_t nframes, const uint32_t* d_seed, uint32_t* d_seg_crc,
                        void* d_out, bool verify, void* stream) {
  if (nframes == 0) return LNX_OK;
  if (!d_first || !d_out) return LNX_EINVAL;
  if (nseg > 0 && (!d_bytes || !d_start || !d_len || !d_seg_crc)) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  hipError_t e = launch_crc32_segments(d_bytes, d_start, d_len, nseg, d_seg_crc, c->d_image, c->num_cus, hs);
  if (e != hipSuccess) return hip_fail(e, "crc32_rows_kernel (segments) launch");
  e = lnxc::launch_chain_fold(d_seg_crc, d_len, nseg, d_first, nframes, d_seed, d_out, verify, c->num_cus, hs);
  if (e != hipSuccess) return hip_fail(e, "chain_fold_kernel launch");
  return LNX_OK;
}

int lnx_crc32_chain_batch(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                          const uint64_t* d_first, uint64_t nframes, const uint32_t* d_seed, uint32_t* d_seg_crc,
                          uint32_t* d_crc, void* stream) {
  return chain_common(d_bytes, d_start, d_len, nseg, d_first, nframes, d_seed, d_seg_crc, d_crc, false, stream);
}

int lnx_fcs_verify_chain_batch(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                               const uint64_t* d_first, uint64_t nframes, uint32_t* d_seg_crc, uint8_t* d_ok,
                               void* stream) {
  return chain_common(d_bytes, d_start, d_len, nseg, d_first, nframes, nullptr, d_seg_crc, d_ok, true, stream);
}

// Two address ranges of a and b bytes share a byte.
static bool ranges_overlap(const void* pa, uint64_t a, const void* pb, uint64_t b) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(pa), y = reinterpret_cast<uintptr_t>(pb);
  return a && b && x < y + b && y < x + a;
}

int lnx_sum_partial_batch(const uint8_t* d_bytes, const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_seed,
                          const uint8_t* d_phase, uint64_t n, uint32_t* d_sum, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_len || !d_sum) return LNX_EINVAL;
  // a row reads seed[i] and writes sum[i]; another row's seed must not have been written yet
  if (d_seed && ranges_overlap(d_seed, n * sizeof(uint32_t), d_sum, n * sizeof(uint32_t))) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxs::launch_sum_bytes(d_bytes, d_off, d_len, d_seed, d_phase, n, d_sum, false, c->num_cus,
                                              static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "sum_bytes_kernel (partial) launch");
  return LNX_OK;
}

int lnx_sum16_chain_batch(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                          const uint64_t* d_first, uint64_t nframes, const uint32_t* d_seed, uint32_t* d_seg_eo,
                          uint16_t* d_out16, uint32_t* d_sum32, void* stream) {
  if (nframes == 0) return LNX_OK;
  if (!d_first || (!d_out16 && !d_sum32)) return LNX_EINVAL;
  if (nseg > 0 && (!d_bytes || !d_start || !d_len || !d_seg_eo)) return LNX_EINVAL;
  // the fold reads the planes while it writes the outputs
  const uint64_t ws = 2 * nseg * sizeof(uint32_t);
  if (nseg > 0 && ((d_out16 && ranges_overlap(d_seg_eo, ws, d_out16, nframes * sizeof(uint16_t))) ||
                   (d_sum32 && ranges_overlap(d_seg_eo, ws, d_sum32, nframes * sizeof(uint32_t)))))
    return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  hipError_t e = lnxs::launch_sum_bytes(d_bytes, d_start, d_len, nullptr, nullptr, nseg, d_seg_eo, true, c->num_cus, hs);
  if (e != hipSuccess) return hip_fail(e, "sum_bytes_kernel (planes) launch");
  e = lnxs::launch_sum_fold(d_seg_eo, d_len, nseg, d_first, nframes, d_seed, d_out16, d_sum32, c->num_cus, hs);
  if (e != hipSuccess) return hip_fail(e, "sum_fold_kernel launch");
  return LNX_OK;
}

int lnx_fcs_append_batch(uint8_t* d_bytes, const uint64_t* d_start, uint32_t* d_len, uint64_t n, uint32_t capacity,
                         uint8_t* d_status, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_start || !d_len || !d_status) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  // one launch of the CRC kernel in its append mode: no scratch, no allocation
  // (a compact CRC array plus a scatter launch measured the same, 0.331 ms:
  // lnx__fcs_append_variant 200)
  const hipError_t e = launch_fcs_append(d_bytes, d_start, d_len, n, capacity, d_status, c->d_image, c->num_cus,
                                         static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "crc32_rows_kernel (append) launch");
  return LNX_OK;
}

#ifdef LNX_RESEARCH
// TX append in two launches (A/B, lnx__fcs_append_variant 200): the segment-mode
// CRC kernel into a compact per-stream scratch, then fcs_scatter_kernel.
static int fcs_append_two_launch(DeviceCtx* c, uint8_t* d_bytes, const uint64_t* d_start, uint32_t* d_len, uint64_t n,
                                 uint32_t capacity, uint8_t* d_status, hipStream_t s) {
  std::lock_guard<std::mutex> lk(c->scratch_mu);  // held until both launches are enqueued
  uint32_t* scr = nullptr;
  int st = stream_scratch(c, s, n * sizeof(uint32_t), reinterpret_cast<void**>(&scr));
  if (st != LNX_OK) return st;
  hipError_t e = launch_crc32_segments(d_bytes, d_start, d_len, n, scr, c->d_image, c->num_cus, s);
  if (e != hipSuccess) return hip_fail(e, "crc32_rows_kernel (append: segments) launch");
  e = launch_fcs_scatter(d_bytes, d_start, d_len, scr, n, capacity, d_status, c->num_cus, s);
  if (e != hipSuccess) return hip_fail(e, "fcs_scatter_kernel launch");
  return LNX_OK;
}
#endif  // LNX_RESEARCH

int lnx_tx_checksum_batch(uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t n,
                          uint8_t* d_status, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_start || !d_len || !d_status) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  // two launches, one of which works (as lnx_ingress_verify_batch): the
  // generate rows, or for a batch whose sampled mean frame is under
  // kTxChecksumShortMean bytes tx_finish with the checksum step only
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  ScratchHold hold;  // until both launches are enqueued
  if ((st = giant_scratch(c, hs, &hold)) != LNX_OK) return st;
  uint32_t* const scratch = hold.p;
  const uint32_t epoch = hold.epoch;
  uint32_t* gate = scratch + kTxChecksumGate;
  hipError_t e = launch_tx_checksum(d_bytes, d_start, d_len, n, d_status, c->num_cus, hs, gate, epoch,
                                    kTxChecksumShortMean);
  if (e != hipSuccess) return hip_fail(e, "tx checksum (ingress_verify_kernel<GEN>) launch");
  e = launch_tx_finish(d_bytes, d_start, const_cast<uint32_t*>(d_len), n, 0, LNX_TX_CHECKSUM, d_status, d_status,
                       c->d_rx, c->num_cus, hs, false, gate, epoch);
  if (e != hipSuccess) return hip_fail(e, "tx_finish_kernel launch");
  return LNX_OK;
}

int lnx_tx_finish_batch(uint8_t* d_bytes, const uint64_t* d_start, uint32_t* d_len, uint64_t n, uint32_t capacity,
                        uint32_t flags, uint8_t* d_status, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_start || !d_len || !d_status) return LNX_EINVAL;
  if ((flags & ~(uint32_t)(LNX_TX_CHECKSUM | LNX_TX_FCS)) != 0) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = launch_tx_finish(d_bytes, d_start, d_len, n, capacity, flags, d_status, d_status, c->d_rx,
                                        c->num_cus, static_cast<hipStream_t>(stream), false);
  if (e != hipSuccess) return hip_fail(e, "tx_finish_kernel launch");
  return LNX_OK;
}

int lnx_crc32_search_batch(const uint8_t* d_bytes, const uint64_t* d_off, const int64_t* d_min_off, uint64_t n,
                           int64_t* d_result, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_result) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  hipError_t e = launch_crc32_search(d_bytes, d_off, d_min_off, n, c->d_search, d_result, c->num_cus,
                                     static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "crc32_search_kernel launch");
  return LNX_OK;
}

int lnx_ingress_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                             uint8_t* d_verdict, void* stream) {
  return lnx_ingress_verify_batch_filtered(d_bytes, d_off, n, flags, nullptr, d_verdict, stream);
}

int lnx_ingress_verify_batch_filtered(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                                      const lnx_rx_filter* filter, uint8_t* d_verdict, void* stream) {
  RxFilter filt;
  if (!rx_filter_of(filter, &filt)) return LNX_EINVAL;
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_verdict) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  // two launches, one of which works (the mean frame length is device-resident):
  // the ingress rows for a batch whose mean frame is >= kIngressShortMean
  // bytes, else the receive check without its CRC (rx_verify_kernel: the same
  // verdicts, no ok output), gated by a word of the stream's scratch
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  ScratchHold hold;  // until both launches are enqueued
  if ((st = giant_scratch(c, hs, &hold)) != LNX_OK) return st;
  uint32_t* const scratch = hold.p;
  const uint32_t epoch = hold.epoch;
  uint32_t* gate = scratch + kIngressGate;
  const uint32_t vf = flags & (LNX_VERIFY_EVIL_BIT | LNX_VERIFY_ICMP);
  hipError_t e = launch_ingress_verify(d_bytes, d_off, n, vf, d_verdict, c->num_cus, hs, nullptr, 0, &filt, gate, epoch,
                                       kIngressShortMean);
  if (e != hipSuccess) return hip_fail(e, "ingress_verify_kernel launch");
  e = launch_rx_verify(d_bytes, d_off, n, vf, false, nullptr, d_verdict, nullptr, &filt, c->d_rx, c->num_cus, hs, false,
                       gate, epoch);
  if (e != hipSuccess) return hip_fail(e, "rx_verify_kernel launch");
  return LNX_OK;
}

int lnx_rx_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                        const lnx_rx_filter* filter, uint8_t* d_fcs_ok, uint8_t* d_verdict, void* stream) {
  RxFilter filt;
  if (!rx_filter_of(filter, &filt)) return LNX_EINVAL;
  if (flags & ~(uint32_t)(LNX_VERIFY_EVIL_BIT | LNX_VERIFY_ICMP | LNX_RX_NO_FCS)) return LNX_EINVAL;
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_fcs_ok || !d_verdict) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = launch_rx_verify(d_bytes, d_off, n, flags & (LNX_VERIFY_EVIL_BIT | LNX_VERIFY_ICMP),
                                        !(flags & LNX_RX_NO_FCS), d_fcs_ok, d_verdict, nullptr, &filt, c->d_rx,
                                        c->num_cus, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "rx_verify_kernel launch");
  return LNX_OK;
}

uint64_t lnx_rx_deliver_ws_bytes(uint64_t n) { return lnxd::deliver_ws_bytes(n); }

// The workspace is the caller's: nothing here touches the per-stream scratch
// sets and their epoch words (giant_scratch), and no device context is needed.
int lnx_rx_deliver_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                         const lnx_rx_filter* filter, const lnx_rx_ports* ports, const uint8_t* d_fcs_ok,
                         const uint8_t* d_verdict, lnx_rx_delivery* d_rec, uint32_t* d_order, uint32_t* d_count,
                         void* d_ws, void* stream) {
  RxFilter filt;
  if (!deliver_args_ok(filter, &filt, flags, LNX_RX_NO_FCS, ports, n, d_rec, d_order, d_count, d_ws)) return LNX_EINVAL;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (n == 0) return zero_words(d_count, LNX_H_COUNT + 1u, hs, "hipMemsetAsync(d_count)");
  if (!d_bytes || !d_off || !d_verdict || !d_rec || (d_order && !d_ws)) return LNX_EINVAL;
  const hipError_t e = lnxd::launch_deliver(d_bytes, d_off, n, (flags & LNX_RX_NO_FCS) ? 0u : 4u, filt, ports, d_fcs_ok,
                                            d_verdict, d_rec, d_order, d_count, d_ws, hs);
  if (e != hipSuccess) return hip_fail(e, "deliver kernels launch");
  return LNX_OK;
}

// The receive check and the delivery records from one read of each frame
// (rx_verify_kernel.hip rv_check with DLV), then the grouping
// launches on the keys it wrote.  As lnx_rx_deliver_batch it works in the
// caller's workspace alone.
int lnx_rx_verify_deliver_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                                const lnx_rx_filter* filter, const lnx_rx_ports* ports, uint8_t* d_fcs_ok,
                                uint8_t* d_verdict, lnx_rx_delivery* d_rec, uint32_t* d_order, uint32_t* d_count,
                                void* d_ws, void* stream) {
  RxFilter filt;
  if (!deliver_args_ok(filter, &filt, flags, LNX_VERIFY_EVIL_BIT | LNX_VERIFY_ICMP | LNX_RX_NO_FCS, ports, n, d_rec, d_order,
                       d_count, d_ws))
    return LNX_EINVAL;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (n == 0) return zero_words(d_count, LNX_H_COUNT + 1u, hs, "hipMemsetAsync(d_count)");
  if (!d_bytes || !d_off || !d_fcs_ok || !d_verdict || !d_rec || (d_order && !d_ws)) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  hipError_t e = lnxd::launch_rx_verify_deliver(d_bytes, d_off, n, flags & (LNX_VERIFY_EVIL_BIT | LNX_VERIFY_ICMP),
                                                !(flags & LNX_RX_NO_FCS), d_fcs_ok, d_verdict, nullptr, &filt, ports,
                                                d_rec, d_order ? lnxd::deliver_keys(d_ws, n) : nullptr, c->d_rx,
                                                c->num_cus, hs);
  if (e != hipSuccess) return hip_fail(e, "rx_verify_deliver_kernel launch");
  if (d_order && (e = lnxd::launch_deliver_group(n, d_order, d_count, d_ws, hs)) != hipSuccess)
    return hip_fail(e, "deliver grouping launches");
  return LNX_OK;
}

uint64_t lnx_rx_rst_ws_bytes(uint64_t n) { return lnxr::rst_ws_bytes(n); }

// RST replies behind the delivery records (reply_kernel.hip).
// The workspace is the caller's, as in the delivery entries; the device context
// gives the table image only.
int lnx_rx_rst_reply_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                           const lnx_rx_delivery* d_rec, const lnx_rst_cfg* cfg, const uint16_t* d_ip_id, uint64_t cap,
                           uint8_t* d_reply, uint32_t* d_src, uint32_t* d_n, void* d_ws, void* stream) {
  if (!reply_args_ok(flags, cfg, n, d_reply, d_rec, d_src, d_n, d_ws, 4, d_ip_id)) return LNX_EINVAL;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (n == 0) return zero_words(d_n, 2, hs, "hipMemsetAsync(d_n)");
  if (!d_bytes || !d_off || !d_rec || !cfg || !d_n || !d_ws) return LNX_EINVAL;
  if (cap > 0 && (!d_ip_id || !d_reply || !d_src)) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  const int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxr::launch_rst_reply(d_bytes, d_off, n, (flags & LNX_RX_NO_FCS) ? 0u : 4u, d_rec, *cfg, d_ip_id,
                                              cap, d_reply, d_src, d_n, d_ws, c->d_rst, hs);
  if (e != hipSuccess) return hip_fail(e, "rst reply kernels launch");
  return LNX_OK;
}

int lnx_tcp_rst_frames_batch(const lnx_rst_cfg* cfg, const lnx_tcp_rst* d_entry, uint64_t n, const uint16_t* d_ip_id,
                             uint8_t* d_reply, void* stream) {
  if (cfg && (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  if (misaligned(d_reply, 64) || misaligned(d_entry, 4) || misaligned(d_ip_id, 2)) return LNX_EINVAL;
  if (n == 0) return LNX_OK;
  if (!cfg || !d_entry || !d_ip_id || !d_reply) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  const int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxr::launch_rst_frames(*cfg, d_entry, n, d_ip_id, d_reply, c->d_rst, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "rst_frames_kernel launch");
  return LNX_OK;
}

uint64_t lnx_rx_echo_ws_bytes(uint64_t n) { return lnxe::echo_ws_bytes(n); }

// Echo replies behind the delivery records (echo_kernel.hip).
// The workspace is the caller's, as in the delivery entries; the device context
// gives the table image only.
int lnx_rx_echo_reply_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                            const lnx_rx_delivery* d_rec, const lnx_rst_cfg* cfg, const uint16_t* d_ip_id,
                            uint64_t cap, uint64_t cap_blocks, uint8_t* d_reply, uint64_t* d_start,
                            uint32_t* d_len, uint32_t* d_src, uint32_t* d_n, void* d_ws, void* stream) {
  if (!reply_args_ok(flags, cfg, n, d_reply, d_rec, d_src, d_n, d_ws, 8, d_ip_id)) return LNX_EINVAL;
  if (misaligned(d_start, 8) || misaligned(d_len, 4)) return LNX_EINVAL;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (n == 0) return zero_words(d_n, 4, hs, "hipMemsetAsync(d_n)");
  if (!d_bytes || !d_off || !d_rec || !cfg || !d_n || !d_ws) return LNX_EINVAL;
  if (cap > 0 && cap_blocks > 0 && (!d_ip_id || !d_reply || !d_start || !d_len || !d_src)) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  const int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxe::launch_echo_reply(d_bytes, d_off, n, (flags & LNX_RX_NO_FCS) ? 0u : 4u, d_rec, *cfg, d_ip_id,
                                               cap, cap_blocks, d_reply, d_start, d_len, d_src, d_n, d_ws, c->d_echo, hs);
  if (e != hipSuccess) return hip_fail(e, "echo reply kernels launch");
  return LNX_OK;
}

uint64_t lnx_rx_arp_ws_bytes(uint64_t n) { return lnxa::arp_ws_bytes(n); }

// ARP replies and learn records behind the delivery records (arp_kernel.hip,
// DESIGN.md §3.22).  The workspace is the caller's, as in the delivery entries;
// the device context gives the table image only (the RST image: the frame is 60
// bytes too).
int lnx_rx_arp_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                     const lnx_rx_delivery* d_rec, const lnx_rst_cfg* cfg, uint64_t cap, uint64_t cap_seen,
                     uint8_t* d_reply, uint32_t* d_src, lnx_arp_seen* d_seen, uint32_t* d_n, void* d_ws, void* stream) {
  if (!reply_args_ok(flags, cfg, n, d_reply, d_rec, d_src, d_n, d_ws, 4, nullptr)) return LNX_EINVAL;
  if (misaligned(d_seen, 16)) return LNX_EINVAL;
  const hipStream_t hs = static_cast<hipStream_t>(stream);
  if (n == 0) return zero_words(d_n, 4, hs, "hipMemsetAsync(d_n)");
  if (!d_bytes || !d_off || !d_rec || !cfg || !d_n || !d_ws) return LNX_EINVAL;
  if ((cap > 0 && (!d_reply || !d_src)) || (cap_seen > 0 && !d_seen)) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  const int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxa::launch_arp_reply(d_bytes, d_off, n, (flags & LNX_RX_NO_FCS) ? 0u : 4u, d_rec, *cfg, cap, cap_seen,
                                              d_reply, d_src, d_seen, d_n, d_ws, c->d_rst, hs);
  if (e != hipSuccess) return hip_fail(e, "arp kernels launch");
  return LNX_OK;
}

int lnx_arp_frames_batch(const lnx_rst_cfg* cfg, const lnx_arp_entry* d_entry, const uint16_t* d_op, uint64_t n,
                         uint8_t* d_reply, void* stream) {
  if (cfg && (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  if (misaligned(d_reply, 64) || misaligned(d_entry, 4) || misaligned(d_op, 2)) return LNX_EINVAL;
  if (n == 0) return LNX_OK;
  if (!cfg || !d_entry || !d_op || !d_reply) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  const int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = lnxa::launch_arp_frames(*cfg, d_entry, d_op, n, d_reply, c->d_rst, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "arp_frames_kernel launch");
  return LNX_OK;
}

int lnx_pcap_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint8_t* d_status,
                          void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_status) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const hipError_t e = launch_pcap_verify(d_bytes, d_off, n, d_status, c->num_cus, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "pcap_verify_kernel launch");
  return LNX_OK;
}

int lnx_crc32_batch_host(const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_off, uint64_t n,
                         uint32_t* h_crc, int device) {
  if (n == 0) return LNX_OK;
  if (!h_bytes || !h_off || !h_crc) return LNX_EINVAL;
  for (uint64_t i = 0; i <= n; ++i)
    if (h_off[i] > nbytes) return LNX_EINVAL;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  uint8_t* d_bytes = nullptr;
  uint64_t* d_off = nullptr;
  uint32_t* d_crc = nullptr;
  int rc = LNX_OK;
  hipStream_t s = nullptr;
  if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e, "hipStreamCreate");
  if ((e = hipMallocAsync(reinterpret_cast<void**>(&d_bytes), nbytes ? nbytes : 4, s)) != hipSuccess ||
      (e = hipMallocAsync(reinterpret_cast<void**>(&d_off), (n + 1) * 8, s)) != hipSuccess ||
      (e = hipMallocAsync(reinterpret_cast<void**>(&d_crc), n * 4, s)) != hipSuccess) {
    rc = hip_fail(e, "hipMallocAsync");
  }
  if (rc == LNX_OK) {
    if ((e = hipMemcpyAsync(d_bytes, h_bytes, nbytes, hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipMemcpyAsync(d_off, h_off, (n + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
      rc = hip_fail(e, "hipMemcpyAsync H2D");
  }
  // (the plain entry: each slice's kernel is picked on the device)
  if (rc == LNX_OK) rc = lnx_crc32_batch(d_bytes, d_off, n, d_crc, s);
  if (rc == LNX_OK && (e = hipMemcpyAsync(h_crc, d_crc, n * 4, hipMemcpyDeviceToHost, s)) != hipSuccess)
    rc = hip_fail(e, "hipMemcpyAsync D2H");
  if (d_bytes) (void)hipFreeAsync(d_bytes, s);
  if (d_off) (void)hipFreeAsync(d_off, s);
  if (d_crc) (void)hipFreeAsync(d_crc, s);
  if ((e = hipStreamSynchronize(s)) != hipSuccess && rc == LNX_OK) rc = hip_fail(e, "hipStreamSynchronize");
  (void)hipStreamDestroy(s);
  return rc;
}

int lnx_crc32_batch_multi(int ngpu, const int* devices, const uint8_t* const* d_bytes_per_gpu,
                          const uint64_t* const* d_off_per_gpu, const uint64_t* n_per_gpu,
                          uint32_t* const* d_crc_per_gpu) {
  if (ngpu <= 0 || !devices || !d_bytes_per_gpu || !d_off_per_gpu || !n_per_gpu || !d_crc_per_gpu)
    return LNX_EINVAL;
  std::vector<int> rcs(ngpu, LNX_OK);
  std::vector<std::string> errs(ngpu);
  std::vector<std::thread> th;
  for (int g = 0; g < ngpu; ++g) {
    th.emplace_back([&, g] {
      hipError_t e = hipSetDevice(devices[g]);
      if (e != hipSuccess) { rcs[g] = hip_fail(e, "hipSetDevice"); errs[g] = g_last_error; return; }
      int rc = lnx_crc32_batch(d_bytes_per_gpu[g], d_off_per_gpu[g], n_per_gpu[g], d_crc_per_gpu[g], nullptr);
      if (rc == LNX_OK && (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, "hipDeviceSynchronize");
      rcs[g] = rc;
      if (rc != LNX_OK) errs[g] = g_last_error;
    });
  }
  for (auto& t : th) t.join();
  for (int g = 0; g < ngpu; ++g)
    if (rcs[g] != LNX_OK) { g_last_error = errs[g]; return rcs[g]; }
  return LNX_OK;
}

#ifdef LNX_RESEARCH
// Profiling hooks of the research library (liblneto_amd_research.so, not in
// include/lneto_amd.h): kernel variants of DESIGN.md §4.
int lnx__crc32_variant(int var, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t* d_crc,
                       void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_crc) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  const rs::StageVariant* sv = rs::stage_variant(var);
  hipError_t e = sv ? rs::launch_crc32_stage_research(d_bytes, d_off, n, d_crc, var & 1, sv->fold, sv->waves, c->d_stage,
                                                      c->num_cus, static_cast<hipStream_t>(stream), sv->big_blocks)
                    : launch_crc32_variant(var, d_bytes, d_off, n, d_crc, c->d_image, c->num_cus,
                                           static_cast<hipStream_t>(stream), nullptr);
  if (e != hipSuccess) return hip_fail(e, "crc32 variant launch");
  return LNX_OK;
}

// Profiling hook: TX FCS append variants (0 = the product, results held and
// flushed; 4 = FCS, length and status stored as each frame finishes).
int lnx__fcs_append_variant(int var, uint8_t* d_bytes, const uint64_t* d_start, uint32_t* d_len, uint64_t n,
                            uint32_t capacity, uint8_t* d_status, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_start || !d_len || !d_status) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  if (var == 200)  // two launches: CRCs into a compact scratch, then the scatter kernel
    return fcs_append_two_launch(c, d_bytes, d_start, d_len, n, capacity, d_status, static_cast<hipStream_t>(stream));
  // 100 (= 0): the one-launch append mode, the product; 4 / 7: its A/B forms
  // (store at once / with the 64-byte sector)
  const hipError_t e = launch_fcs_append(d_bytes, d_start, d_len, n, capacity, d_status, c->d_image, c->num_cus,
                                         static_cast<hipStream_t>(stream), var == 100 ? 0 : var);
  if (e != hipSuccess) return hip_fail(e, "fcs append variant launch");
  return LNX_OK;
}

// Profiling hook: sum16 kernel variants (0 = line rows, the product; 1 = the
// r1c half-line rows).
int lnx__sum16_variant(int var, const uint8_t* d_bytes, const uint64_t* d_off, const uint32_t* d_len,
                       const uint32_t* d_seed, uint64_t n, uint16_t* d_out, void* stream) {
  if (n == 0) return LNX_OK;
  if (!d_bytes || !d_off || !d_len || !d_out) return LNX_EINVAL;
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  hipError_t e = launch_sum16_segments(d_bytes, d_off, d_len, d_seed, n, d_out, c->num_cus,
                                       static_cast<hipStream_t>(stream), var);
  if (e != hipSuccess) return hip_fail(e, "sum16 variant launch");
  return LNX_OK;
}

// Profiling hook: the variant with a per-wave timeline (3 x uint64 per wave:
// entry, image copied, exit; 100 MHz clock).  Returns the wave count when
// d_timeline is NULL.
int64_t lnx__crc32_timeline(int var, const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t* d_crc,
                            uint64_t* d_timeline, void* stream) {
  DeviceCtx* c = nullptr;
  int st = get_ctx(&c);
  if (st != LNX_OK) return st;
  if (!d_timeline) return (int64_t)crc32_launch_waves(n, c->num_cus);
  if (n == 0 || !d_bytes || !d_off || !d_crc) return LNX_EINVAL;
  hipError_t e = launch_crc32_variant(var, d_bytes, d_off, n, d_crc, c->d_image, c->num_cus,
                                      static_cast<hipStream_t>(stream), d_timeline);
  if (e != hipSuccess) return hip_fail(e, "crc32 timeline launch");
  return LNX_OK;
}
#endif  // LNX_RESEARCH

int lnx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* lnx_last_error(void) { return g_last_error.c_str(); }

const char* lnx_version(void) {
  return "lneto_amd 0.13 gfx950: crc32 rows (32-lane whole-line rows from 4096 B mean: 24-line items; one-word "
         "16-lane rows 1600-4096 B: 1 slot x 24 steps, 4-frame chunks; lean two-word line rows 640-1600 B, offsets "
         "and segment mode: one 13-line frame per row per slot; whole-line rows load a frame's first and last lines "
         "at the default cache policy, the rest nt; 4-lane rows: 2 slots x 16 steps, 32-frame chunks, held results; "
         "narrow rows load only the 4-step runs an item has; TX FCS append in the same launch: pad, FCS, length, "
         "status; segment slices out of address order folded frame by frame) + sum16 16-lane line rows + ingress "
         "verdicts (qword rows, end mask on the last qword, ICMP clients' checks) and TX checksum generate (the same "
         "rows, GEN) + rx ring (ingress and egress packets) + CRC32Search (eight captures per wave, 192-byte lane "
         "segments as four 48-byte chains joined by lane-private Z_48 nibble tables, 3-level scan, Z_4 in the "
         "lane-private U layout, pass B by word checks, group-descriptor loads) + staged lane streams for "
         "short-frame batches (slicing-by-8 fold, LDS transposed whole-line loads; out-of-order blocks by lane and "
         "by whole waves) and slice dispatch on the device (staged launch gated by the rows launch's flag word; "
         "giant slices by span, mean or 8x skew, out-of-order giant slices frame by frame) + rx_verify (FCS and "
         "verdicts in one read: 16-lane rows, 56-frame groups, the next pass loaded ahead, units no frame reaches "
         "skipped) + tx_finish (checksums, padding and FCS in one read, CRC corrected by linearity; 16 waves, "
         "48-frame groups) + zero copy through the ring's pinned slots + running CRCs (seeds, "
         "combine, frames made of segments: Z_k by nibble tables of x^(8 * 2^j) in LDS, a 16-lane row or the "
         "workgroup per frame) + running internet checksums (raw 32-bit sums at either byte phase, frames made of "
         "segments: the sum16 line rows into E / O planes, a 16-lane row or the workgroup's four waves per frame) + "
         "receive delivery (the port stage: a 16-lane row per frame, header bytes only, port tables in LDS; frames "
         "grouped by handler in arrival order by a counting sort over contiguous slices) + receive check and "
         "delivery records in one read (the receive kernel's frame lane applies the port stage to its staged "
         "header; the ring's deliver entries on every route)";
}

}  // extern "C"
