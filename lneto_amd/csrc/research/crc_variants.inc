// crc_variants.inc — the research library's crc32_rows_kernel variants
// (included in crc32_kernel.hip under LNX_RESEARCH, after launch_cfg): the ids
// lnx__crc32_variant / lnx__crc32_timeline / lnx__fcs_append_variant take
// (tools/prof/variants.py, tools/prof/append_ab.py; DESIGN.md §4).  Every
// variant is a product configuration (rows_cfg.hpp) with the fields it names
// changed.  Ids 80 / 81 change the grid, not the kernel (launch_crc32_variant);
// 300-342 are the staged kernel's (launch.hpp kStageVariants).

// VARIANT(base, c.field = value, ...): launch `base` with those fields changed
#define VARIANT(BASE, ...) launch_cfg<with(BASE, [](RowsCfg& c) { __VA_ARGS__; })>(a)

// The offsets product with the 4-lane rows of the round before it (those of
// kRowsSegments): what the variants up to id 93 were measured against.
inline constexpr RowsCfg kRowsOld4 = with(kRowsOffsets, [](RowsCfg& c) { c.ks4 = 12, c.ch4 = 16; });

// Offsets mode, CRC: launches variant `var`; false (nothing launched) when
// `var` is none of the table's: the caller launches the product.
inline bool launch_offsets_variant(int var, const RowsArgs& a) {
  switch (var) {
    case 1: VARIANT(kRowsOffsets, c.probe = Probe::kLoadsOnly); break;
    case 2: VARIANT(kRowsOffsets, c.probe = Probe::kMathOnly); break;
    case 3: VARIANT(kRowsOffsets, c.probe = Probe::kWindow64); break;
    case 5: VARIANT(kRowsOffsets, c.probe = Probe::kFlush4); break;
    // forced 32-lane rows
    case 10: VARIANT(kRowsOld4, c.width = Width::k32, c.ksw = 13); break;  // one 13-line item per 1500 B
    case 11: VARIANT(kRowsOld4, c.width = Width::k32, c.ksw = 13, c.sw = 2); break;  // two-slot ring
    case 12: VARIANT(kRowsOld4, c.width = Width::k32, c.ksw = 14); break;
    case 13: VARIANT(kRowsOld4, c.width = Width::k32, c.ksw = 13, c.chw = 2); break;  // 2-frame chunks
    case 14: VARIANT(kRowsOld4, c.width = Width::k32, c.ksw = 13, c.chw = 8); break;  // 8-frame chunks
    case 15: VARIANT(kRowsOld4, c.width = Width::k32); break;  // 24-line items
    case 16: VARIANT(kRowsOld4, c.width = Width::k32, c.ksw = 18); break;
    // forced 16-lane rows, one word per lane
    case 17: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kOneWord); break;  // round-1 product
    case 21: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kOneWord, c.ksm = 12, c.sm = 3); break;
    // forced 16-lane rows, two words per lane
    case 18: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 13); break;  // one 13-line item per 1500 B
    case 19: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 13, c.sm = 2); break;  // two-slot ring
    case 28: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 14); break;
    case 29: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords); break;  // 24-line items
    case 43: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 32); break;  // 32-line items
    case 44: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 18); break;
    case 40: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 13, c.chm = 8); break;  // 8-frame chunks
    case 41: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 12, c.sm = 2); break;
    case 42: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kTwoWords, c.ksm = 13, c.chm = 16); break;
    // forced lean line rows (lines_body)
    case 50: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean); break;
    case 51: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.ksl = 14); break;
    case 52: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.ksl = 12); break;
    case 53: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.probe = Probe::kLoadsOnly); break;
    case 54: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.probe = Probe::kMathOnly); break;
    // forced lean rows on 32 lanes x one word
    case 70: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.lwl = 1); break;
    case 71: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.lwl = 1, c.probe = Probe::kLoadsOnly); break;
    case 72: VARIANT(kRowsOld4, c.width = Width::k16, c.mid = Mid::kLean, c.lwl = 1, c.probe = Probe::kMathOnly); break;
    // product dispatch with one-word 16-lane rows instead of lean rows (the r1f product)
    case 56: VARIANT(kRowsOld4, c.mid = Mid::kOneWord); break;
    // the product dispatch with the r1 lean rows (junk word reloaded, its U-image taken out), and its loads only
    case 57: VARIANT(kRowsOld4, c.ljm = false); break;
    case 58: VARIANT(kRowsOld4, c.ljm = false, c.probe = Probe::kLoadsOnly); break;
    // lean rows by the cache policy of their step loads (RowsCfg::lep): all nt (the r2b product) and
    // its loads only, the first step at the default policy, every step at the default policy
    case 90: VARIANT(kRowsOld4, c.lep = 0); break;
    case 91: VARIANT(kRowsOld4, c.lep = 0, c.probe = Probe::kLoadsOnly); break;
    case 92: VARIANT(kRowsOld4, c.lep = 2); break;
    case 93: VARIANT(kRowsOld4, c.lep = 3); break;
    // the product dispatch with 32-lane line rows all nt (the r1 form)
    case 97: VARIANT(kRowsOffsets, c.redge = false); break;
    // forced 4-lane rows (24 = 62 and 22 = 63: the same instance under two ids)
    case 22: case 63: VARIANT(kRowsOffsets, c.width = Width::k4); break;
    case 23: VARIANT(kRowsOffsets, c.width = Width::k4, c.ks4 = 8, c.s4 = 3, c.ch4 = 64); break;
    case 24: case 62: VARIANT(kRowsOffsets, c.width = Width::k4, c.ks4 = 12); break;
    case 25: VARIANT(kRowsOffsets, c.width = Width::k4, c.ks4 = 6, c.s4 = 3, c.ch4 = 64); break;
    case 60: VARIANT(kRowsOffsets, c.width = Width::k4, c.ch4 = 16); break;  // longer 4-lane items
    case 61: VARIANT(kRowsOffsets, c.width = Width::k4, c.ks4 = 20, c.s4 = 1, c.ch4 = 16); break;
    case 64: VARIANT(kRowsOffsets, c.width = Width::k4, c.ks4 = 12, c.ch4 = 64); break;
    case 65: VARIANT(kRowsOffsets, c.width = Width::k4, c.ch4 = 64); break;
    case 26: VARIANT(kRowsOffsets, c.width = Width::k4, c.probe = Probe::kLoadsOnly); break;
    case 27: VARIANT(kRowsOffsets, c.width = Width::k4, c.probe = Probe::kMathOnly); break;
    // narrow and one-word 16-lane rows by the runs their item loads (RowsCfg::nsr4): 125 every step of
    // the item (the r2 product: a short last item reads the next frames' bytes), 124 / 120 / 126
    // runs of 1 / 2 / 6 steps (the product: 4; r2ze/r2zf Zipf 1.057 ms against 1.071 for 2, 1.077
    // for every step, 1.056 for 6)
    case 125: VARIANT(kRowsOffsets, c.nsr4 = 0); break;
    case 120: VARIANT(kRowsOffsets, c.nsr4 = 2); break;
    case 124: VARIANT(kRowsOffsets, c.nsr4 = 1); break;
    case 126: VARIANT(kRowsOffsets, c.nsr4 = 6); break;
    // four-word 4-lane rows (dwordx4: 64 contiguous bytes per row instruction) under the product
    // dispatch: ks4 steps of 64 B, s4 slots, ch4-frame chunks, nsr4-step load runs
    case 130: VARIANT(kRowsOffsets, c.nw4 = 4, c.ks4 = 4, c.nsr4 = 1); break;
    case 135: VARIANT(kRowsOffsets, c.nw4 = 4, c.ks4 = 4, c.nsr4 = 1, c.probe = Probe::kLoadsOnly); break;
    case 136: VARIANT(kRowsOffsets, c.nw4 = 4, c.ks4 = 4, c.nsr4 = 1, c.probe = Probe::kMathOnly); break;
    case 138: VARIANT(kRowsOffsets, c.nw4 = 4, c.ks4 = 4, c.nsr4 = 1, c.ch4 = 16); break;
    case 139: VARIANT(kRowsOffsets, c.nw4 = 4, c.ks4 = 3, c.nsr4 = 1); break;
    case 140: VARIANT(kRowsOffsets, c.nw4 = 4, c.ks4 = 5, c.nsr4 = 1); break;
    // streaming rows (research/stream_rows.hpp) for the narrow rows' frames, under the product
    // dispatch: full, loads + chain only, loads only
    case 150: VARIANT(kRowsOffsets, c.stream = Stream::kRows8); break;
    case 151: VARIANT(kRowsOffsets, c.stream = Stream::kRows8, c.probe = Probe::kStreamChain); break;
    case 152: VARIANT(kRowsOffsets, c.stream = Stream::kRows8, c.probe = Probe::kStreamLoads); break;
    // the same on 4-lane rows
    case 153: VARIANT(kRowsOffsets, c.stream = Stream::kRows4); break;
    case 154: VARIANT(kRowsOffsets, c.stream = Stream::kRows4, c.probe = Probe::kStreamChain); break;
    case 155: VARIANT(kRowsOffsets, c.stream = Stream::kRows4, c.probe = Probe::kStreamLoads); break;
    // lane streams (research/stream_lanes.hpp)
    case 160: VARIANT(kRowsOffsets, c.stream = Stream::kLanes); break;
    case 161: VARIANT(kRowsOffsets, c.stream = Stream::kLanes, c.probe = Probe::kLanesLoads); break;
    case 162: VARIANT(kRowsOffsets, c.stream = Stream::kLanes, c.probe = Probe::kLanesChain); break;
    case 164: VARIANT(kRowsOffsets, c.stream = Stream::kLanes, c.probe = Probe::kLanesFoldReset); break;
    case 165: VARIANT(kRowsOffsets, c.stream = Stream::kLanes, c.probe = Probe::kLanesHalfOffsets); break;
    default: return false;
  }
  return true;
}

// The TX FCS append's A/B forms (lnx__fcs_append_variant 4 / 7); false: the product.
inline bool launch_append_variant(int var, const RowsArgs& a) {
  switch (var) {
    case 4: VARIANT(kRowsSegments, c.mode = CrcMode::kAppend, c.probe = Probe::kStoreAtOnce); break;
    case 7: VARIANT(kRowsSegments, c.mode = CrcMode::kAppend, c.probe = Probe::kSectorStore); break;
    default: return false;
  }
  return true;
}
#undef VARIANT
