// rows_cfg.hpp — which crc32_rows_kernel is built: the kernel's one template
// argument (crc32_kernel.hip), the two product configurations, and the names
// of the profiling probes.  The research library's variants
// are these configurations with some fields changed (research/crc_variants.inc).
#pragma once

namespace lnx {

// kAppend: segment mode only (crc32_kernel.hip, the TX FCS append)
enum class CrcMode : int { kCrc = 0, kVerify = 1, kAppend = 2 };

// Profiling probes (research library only; the numbers are the ones the
// profiles and DESIGN.md §4 use).  Only kProduct is reachable from the C-ABI.
enum class Probe : int {
  kProduct = 0,
  kLoadsOnly = 1,     // loads + bookkeeping only
  kMathOnly = 2,      // lookups + bookkeeping on synthetic words
  kWindow64 = 3,      // the bounds window loaded by all 64 lanes (the earlier behaviour)
  kStoreAtOnce = 4,   // kAppend: FCS, length and status stored as each frame finishes, no hold
  kFlush4 = 5,        // clock-window flushes for 4-lane rows too
  kSectorStore = 7,   // kAppend, two-word rows: the FCS written with its 64-byte sector
  // streaming rows (research/stream_rows.hpp)
  kStreamChain = 151,  // loads + chain only (no frame boundaries)
  kStreamLoads = 152,  // loads only
  // lane streams (research/stream_lanes.hpp)
  kLanesLoads = 161,       // loads only
  kLanesChain = 162,       // loads + chain only
  kLanesFoldReset = 164,   // the reset as a select inside the fold
  kLanesHalfOffsets = 165  // kLanesFoldReset + offset requests on even sets only
};

// What folds the narrow rows' frames in offsets mode when the slice's bytes fit
// 31-bit buffer offsets from a line-aligned base (research library only).
enum class Stream : int {
  kNone = 0,   // the product: rows_body
  kRows8 = 1,  // streaming rows, 8 lanes: one 128-byte line per row step
  kRows4 = 2,  // streaming rows, 4 lanes: 64-byte row steps, at most one boundary per step
  kLanes = 3   // lane streams
};

// The row width: chosen per workgroup from its slice's mean frame length, or
// forced for the whole launch (research library only).
enum class Width : int { kPerSlice = 0, k4 = 4, k16 = 16, k32 = 32 };

// What the 16-lane rows (slices of kShortMean..kLineMean bytes a frame) run.
// (24-line lean items for 1600-3000 B were tried: w[24] pushed the kernel past
// its VGPR budget into scratch.)
enum class Mid : int {
  kOneWord = 1,   // one word per lane
  kTwoWords = 2,  // two words per lane: a row reads a whole line per instruction
  kLean = 3,      // lean line rows (lines_body)
  kLeanShort = 4  // lean line rows below kLeanMean, one word per lane above
};

// One crc32_rows_kernel instance.  (mode, probe and stream come first, and a
// non-zero field follows them: the mangled name of a class-type template
// argument lists the members in order and drops trailing zeros, so every
// instance's symbol shows the three; tests/test_abi.py reads them there.)
struct RowsCfg {
  CrcMode mode;
  Probe probe;
  Stream stream;
  Width width;
  // 32-lane rows (whole 128-byte lines, slices of kLineMean bytes a frame and more)
  int ksw;  // window steps (lines) per item
  int sw;   // ring slots
  // 4-lane rows (slices under kShortMean bytes a frame)
  int ks4;  // window steps per item
  int s4;   // ring slots
  int chw;  // 32-lane rows: frames per chunk claimed from the LDS counter
  int ch4;  // 4-lane rows: the same
  // segment mode: frame i = bytes[start[i] : start[i] + len[i]], in address
  // order, not overlapping (ring slots, lnx_crc32_segments, the TX FCS append)
  bool seg;
  Mid mid;
  // one- and two-word 16-lane rows
  int ksm;  // window steps per item
  int sm;   // ring slots
  int chm;  // frames per chunk
  // lean line rows (lines_body)
  int ksl;   // lines per item
  int lwl;   // words per lane: 2 = 16 lanes a row, 1 = 32 lanes a row
  bool ljm;  // junk bytes after the frame end masked in the fold (false: the word reloaded, its U-image taken out)
  int lep;   // step loads at the default cache policy: 0 none (all nt), 1 the first and the last two, 2 the first, 3 all
  // 32-lane rows: an item's first step and its last two at the default cache
  // policy, so the line two frames share is fetched once (false: all nt)
  bool redge;
  // 4-lane and one-word 16-lane rows: an item's loads issued in runs of this
  // many steps it has (0: every step of the item, where a short last item
  // reads the next frames' bytes)
  int nsr4;
  int nw4;  // 4-lane rows: words per lane (4: dwordx4, 64 contiguous bytes per row instruction)
};

// offsets mode (lnx_crc32_batch, lnx_fcs_verify_batch)
inline constexpr RowsCfg kRowsOffsets = {
    .mode = CrcMode::kCrc, .probe = Probe::kProduct, .stream = Stream::kNone, .width = Width::kPerSlice,
    .ksw = 24, .sw = 1, .ks4 = 16, .s4 = 2, .chw = 4, .ch4 = 32, .seg = false, .mid = Mid::kLeanShort,
    .ksm = 24, .sm = 1, .chm = 4, .ksl = 13, .lwl = 2, .ljm = true, .lep = 1, .redge = true, .nsr4 = 4, .nw4 = 1};

// A configuration with some fields changed: with(kRowsOffsets, [](RowsCfg& c) { c.mode = CrcMode::kVerify; })
template <class F>
constexpr RowsCfg with(RowsCfg c, F change) {
  change(c);
  return c;
}

constexpr RowsCfg in_mode(RowsCfg c, CrcMode mode) {
  c.mode = mode;
  return c;
}

// segment mode (lnx_crc32_segments, the TX FCS append, the receive ring): the
// 4-lane rows of the round before the offsets product's
inline constexpr RowsCfg kRowsSegments = with(kRowsOffsets, [](RowsCfg& c) { c.seg = true, c.ks4 = 12, c.ch4 = 16; });

}  // namespace lnx
