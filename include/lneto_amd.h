/*
 * lneto_amd.h — C-ABI of the MI355X-native checksum path of lneto.
 *
 * Scope: the IEEE 802.3 CRC-32 frame-check-sequence
 * (lneto ethernet/crc.go) and the RFC 791 16-bit one's-complement internet
 * checksum (lneto crc.go, type CRC791).  Everything here is integer / byte
 * arithmetic and bit-identical to the reference.
 *
 * Two families of entry points:
 *
 *  1. Per-frame, host-CPU, exact Go semantics.  These back the drop-in
 *     replacements of the reference's single-frame functions and NEVER launch
 *     a GPU kernel (a launch costs microseconds, a 64-byte CRC costs tens of
 *     nanoseconds; SURVEY.md §7 "cgo/HIP boundary").
 *
 *  2. Batched, device-resident, HIP kernels for gfx950.  Frames are packed back
 *     to back in one device buffer and described by N+1 uint64 byte offsets:
 *     frame i is bytes[off[i] : off[i+1]].  These are the hot path.
 *
 * Conventions (mirroring the reference):
 *  - the caller owns every buffer; nothing is retained after a call returns;
 *  - batch entry points return LNX_OK (0) or a negative LNX_E* code and never
 *    abort; per-frame checksum functions return values, never errors;
 *  - `stream` is a hipStream_t passed as an opaque pointer (NULL = the null
 *    stream of the current device); batch calls are asynchronous on it;
 *  - batch entry points may be called from any number of host threads at once,
 *    on the same stream or on different ones.  Calls that several threads make
 *    on one stream take effect in some order, each call whole (its launches
 *    are never interleaved with another call's on that stream); calls on
 *    different streams never wait for each other's device work.  The caller
 *    still orders what it must: a call that reads what another wrote goes
 *    after it on the stream.
 */
#ifndef LNETO_AMD_H
#define LNETO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define LNX_OK 0
#define LNX_EINVAL (-1)    /* bad argument (NULL pointer with n > 0, ...) */
#define LNX_ENODEV (-2)    /* no HIP device / bad device ordinal */
#define LNX_EHIP (-3)      /* a HIP runtime call failed; see lnx_last_error() */
#define LNX_ENOMEM (-5)

/* CRC-32/ISO-HDLC residue: CRC32(frame || LE32(CRC32(frame))) == this value. */
#define LNX_CRC32_RESIDUE 0x2144DF1Cu

/* ======================================================================== *
 * 1. Per-frame host functions (exact Go semantics, never touch the GPU)
 * ======================================================================== */

/* Go: crc32.Update(crc, crc32.IEEETable, p) — the CRC32Update plugin hook
 * type of internet.StackEthernetConfig (internet/stack-ethernet.go:31-32),
 * surfaced as xnet.StackConfig.EthernetTxCRC32Update (x/xnet/stack-async.go:89)
 * and called at internet/stack-ethernet.go:211-214. */
uint32_t lnx_crc32_update(uint32_t crc, const uint8_t* p, size_t n);

/* Go: ethernet.CRC32(data) (ethernet/crc.go:19-21). CRC32(nil) == 0. */
uint32_t lnx_crc32(const uint8_t* p, size_t n);

/* CRC32(A || B) from CRC32(A), CRC32(B) and len(B), exact for every 64-bit
 * length (zlib's crc32_combine):
 *   lnx_crc32_combine(lnx_crc32(A), lnx_crc32(B), |B|) == lnx_crc32(A || B),
 *   lnx_crc32_combine(seed, lnx_crc32(B), |B|) == lnx_crc32_update(seed, B).
 * Joins CRCs taken over pieces of a frame, in other launches or on other
 * devices; associative, identity (crc 0, length 0). */
uint32_t lnx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* Go: ethernet.CRC32Search(data, minOffCRC) (ethernet/crc.go:28-47).
 * First off >= max(minOff,0) with CRC32(data[:off]) == LE32(data[off:]),
 * or -1.  The result is -1 for every int64 min_off above n - 4 (Go panics on
 * a minOffCRC past the data; no sum of min_off overflows here). */
int64_t lnx_crc32_search(const uint8_t* p, size_t n, int64_t min_off);

/* Go: sumWriteEven (crc.go:23-28) — uint32 wrap-around sum of big-endian
 * 16-bit words.  n must be even (the Go method panics on odd length, crc.go:30);
 * here an odd trailing byte is ignored and the caller is expected not to pass one. */
uint32_t lnx_sum_write_even(uint32_t sum, const uint8_t* p, size_t n);

/* Go: sum16 (crc.go:17-21) — CRC791.Sum16() of a running sum. */
uint16_t lnx_sum16(uint32_t sum);

/* Go: CRC791{sum}.PayloadSum16(p) (crc.go:52-59). */
uint16_t lnx_sum16_payload(uint32_t sum, const uint8_t* p, size_t n);

/* The raw running sum of CRC791 (crc.go:13-62) over a piece of a packet: with
 * E / O = the sums of p's bytes at even / odd offsets from p,
 *   phase & 1 == 0:  sum + 256 E + O   (the piece starts at an even offset of its packet),
 *   phase & 1 == 1:  sum + E + 256 O   (at an odd offset: the halves of every word swap),
 * mod 2^32 as the reference's uint32 wraps (crc.go:23-28); an odd last byte is
 * an even-offset byte, the `<< 8` of crc.go:56.  With phase 0 and even n this is
 * lnx_sum_write_even (WriteEven, crc.go:30-33); lnx_sum16 of the result with
 * phase 0 is lnx_sum16_payload (crc.go:52-59).  A checksum over data that
 * arrives in pieces passes each call the sum so far and phase = the bytes so
 * far & 1. */
uint32_t lnx_sum_partial(uint32_t sum, const uint8_t* p, size_t n, int phase);

/* CRC791{seed}.PayloadSum16 (crc.go:52-59) over the concatenation of m
 * buffers seg[k][0 : len[k]] (a header buffer plus a payload buffer, a frame
 * in several ring slots); empty buffers (their pointers are not read) and
 * m == 0 (sum16 of the seed, crc.go:17-21) are valid. */
uint16_t lnx_sum16_chain(uint32_t seed, const uint8_t* const* seg, const size_t* len, size_t m);

/* Go: lneto.NeverZeroSum (crc.go:65-71). */
uint16_t lnx_never_zero_sum(uint16_t sum16);

/* The receive path's checksum-stage verdict of ONE Ethernet frame (FCS
 * stripped) on the host: the value lnx_ingress_verify_batch_filtered computes
 * per frame (StackEthernet.Demux, internet/stack-ethernet.go:139-165, then
 * demux4 / demux6, internet/stack-ip4.go:100-164, internet/stack-ip6.go:86-138;
 * codes and flags as documented there; filter NULL = accept-all).  Returns the
 * verdict (>= 0) or LNX_EINVAL.  The packet entries (lnx_ingress_packets,
 * lnx_rx_ring_ingress) use it for batches below their host threshold, so
 * netdev's one-buffer-per-call Runner (x/netdev/runner.go:432-433) never
 * launches a kernel. */
#define LNX_VERIFY_EVIL_BIT 1u /* lneto.ValidateEvilBit on the stack's Validator */
#define LNX_VERIFY_ICMP 2u     /* the ICMPv4 / ICMPv6 clients are attached (StackAsync.EnableICMP) */
struct lnx_rx_filter;
int lnx_ingress_verdict(const uint8_t* frame, size_t len, uint32_t flags, const struct lnx_rx_filter* filter);

/* pcap's checksum re-verification of ONE Ethernet frame on the host: what
 * PacketBreakdown.CaptureEthernet records about the frame's checksums
 * (internet/pcap/capture.go:67-277), which differs from the receive path's
 * verdict: a bad IPv4 header sum is recorded and the transport check still
 * runs (:229-231); on IPv4 the TCP / UDP checks run only when tcp / udp.NewFrame
 * accept the payload (:241-266), a UDP checksum of 0 is not checked (:259),
 * ICMPv4 is always summed with no pseudo-header (:267-273); IPv6 sums UDP and
 * UDPLite over the UDP length (:184-198).  Returns the status byte (>= 0):
 * LNX_PCAP_IP_HDR_BAD | LNX_PCAP_PROTO_BAD | code << 2, code = the errGeneric
 * value (15 ErrInvalidLengthField, 18 ErrTruncatedFrame) of a size check that
 * ends the capture on the way to the transport check (IPv6 UDP / UDPLite: the
 * error pcap records in its place), else 0; or LNX_EINVAL.  802.3 length
 * frames, VLAN-tagged frames and other EtherTypes have no checksum stage in
 * pcap (status 0 unless their Ethernet size check fails). */
#define LNX_PCAP_IP_HDR_BAD 1u /* ErrBadCRC in the IPv4 frame's Errors */
#define LNX_PCAP_PROTO_BAD 2u  /* ipProtoErr == ErrBadCRC (the transport frame's Errors) */
int lnx_pcap_checksums(const uint8_t* frame, size_t len);

/* The transmit checksum step of ONE frame on the host, in place: the per-frame
 * semantics of lnx_tx_checksum_batch (encapsulate4 / encapsulate6 / the ICMP
 * clients, internet/stack-ip4.go:202-228, internet/stack-ip6.go:167-181).
 * Returns the status (0, 18 ErrTruncatedFrame, 15 ErrInvalidLengthField) or
 * LNX_EINVAL. */
int lnx_tx_checksum(uint8_t* frame, size_t len);

/* StackEthernet.Encapsulate's tail with the CRC32Update hook set, ONE frame on
 * the host (internet/stack-ethernet.go:200-214): zero-pad to 60 bytes, append
 * the LE FCS, *len = the new length; 6 (ErrShortBuffer) with the frame
 * untouched when it would outgrow `capacity`; LNX_EINVAL for NULL pointers. */
int lnx_fcs_append(uint8_t* frame, uint32_t* len, uint32_t capacity);

/* ======================================================================== *
 * 2. Batched device-resident HIP path (gfx950)
 * ======================================================================== */

/* d_crc[i] = CRC32(d_bytes[d_off[i] : d_off[i+1]]) for i in [0, n).
 * d_off holds n+1 offsets, non-decreasing for the fast paths; offsets out of
 * order are accepted too (a frame whose end offset is below its start is
 * treated as empty, CRC 0; every other frame, overlapping ones included, gets
 * the CRC of its own bytes: a workgroup slice with a decreasing pair of
 * offsets is folded frame by frame, each from its own start).  One exception:
 * in a batch of more than 1024 frames per compute unit a slice (the frames of
 * one workgroup) has every pair of its offsets looked at only if one of the 64
 * frames sampled over it has its end below its start or if all 64 have 4096
 * bytes or more.  Otherwise (the 64 in order, one under 4096 bytes) the sample
 * decides alone, and a frame elsewhere in that slice that reaches outside
 * [d_off of the slice's first frame, d_off of its end] gets the CRC of its
 * bytes inside that range with zeros for the rest (looking
 * at every pair costs 0.4 % at 1500 B there).  Frames may have any length and
 * any byte alignment.  Each workgroup slice's kernel is picked on the device
 * from its offsets, so the call never reads device memory on
 * the host and never syncs.  Replaces n calls of ethernet.CRC32
 * (ethernet/crc.go:19-21) / of the CRC32Update hook
 * (internet/stack-ethernet.go:211-214; its crc argument:
 * lnx_crc32_update_batch). */
int lnx_crc32_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n,
                    uint32_t* d_crc, void* stream);

/* lnx_crc32_batch / lnx_fcs_verify_batch with flags.  LNX_BATCH_SHORT_FRAMES
 * forces the staged lane-stream kernel (each 128-byte line
 * requested once) for every slice that is not giant, where the plain entries
 * let the device pick per slice (uniform lengths the rows kernel is faster at
 * go to it).  Results are identical either way.  Other bits must be 0. */
#define LNX_BATCH_SHORT_FRAMES 1u
int lnx_crc32_batch_ex(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t* d_crc, uint32_t flags,
                       void* stream);
int lnx_fcs_verify_batch_ex(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint8_t* d_ok,
                            uint32_t flags, void* stream);

/* Segment form of lnx_crc32_batch for frames that are not packed back to back
 * (ring slots): d_crc[i] = CRC32(d_bytes[d_start[i] : d_start[i] + d_len[i]]).
 * Any order, overlap allowed.  Frames in increasing address order that do not
 * overlap take the pipelined rows; a workgroup slice that is not
 * (start[i] + len[i] > start[i + 1] somewhere) is folded frame by frame, each
 * from its own start. */
int lnx_crc32_segments(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t n,
                       uint32_t* d_crc, void* stream);

/* ---- running CRCs: seeds, combine, frames made of segments ----
 * As every batch entry these are asynchronous on `stream`, never sync, never
 * read device memory on the host, never allocate and retain nothing (hence the
 * caller's workspace below).  A zero count (n, nframes) returns LNX_OK; a NULL
 * required pointer with a non-zero count LNX_EINVAL; no usable device
 * LNX_ENODEV / LNX_EHIP. */

/* d_out[i] = lnx_crc32_combine(d_crc_a[i], d_crc_b[i], d_len_b[i]) for i in
 * [0, n).  d_out may alias d_crc_a or d_crc_b. */
int lnx_crc32_combine_batch(const uint32_t* d_crc_a, const uint32_t* d_crc_b, const uint64_t* d_len_b, uint64_t n,
                            uint32_t* d_out, void* stream);

/* The CRC32Update hook with its crc argument (internet/stack-ethernet.go:31-32):
 * d_crc[i] = CRC32Update(d_seed[i], d_bytes[d_off[i] : d_off[i+1]]), offsets as
 * lnx_crc32_batch (an end offset below its start is an empty frame: its result
 * is the seed itself).  d_seed NULL = all-zero seeds, then identical to
 * lnx_crc32_batch (and no further launch); else lnx_crc32_batch's launches
 * into d_crc and one launch that folds the seeds in.  d_seed and d_crc must
 * not overlap: the host compares the two address ranges and returns LNX_EINVAL
 * if they do.  A running CRC over several calls (data that arrives in pieces)
 * ping-pongs two arrays: call k reads the array call k-1 wrote and writes the
 * other. */
int lnx_crc32_update_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, const uint32_t* d_seed,
                           uint32_t* d_crc, void* stream);

/* Frames made of segments (a jumbo frame in several ring slots, a header
 * buffer plus a payload buffer): frame f is the concatenation, in index order,
 * of segments d_first[f] .. d_first[f+1]-1; segment k is
 * d_bytes[d_start[k] : d_start[k] + d_len[k]].
 *   d_crc[f] = CRC32Update(d_seed ? d_seed[f] : 0, frame f).
 * Segments may lie in any address order, overlap (as lnx_crc32_segments) and
 * be empty.  A frame with d_first[f+1] <= d_first[f] has no segments: its CRC
 * is its seed (0 without one).  d_first holds nframes+1 entries and the caller
 * keeps d_first[nframes] <= nseg; the kernel still clamps every segment index
 * to nseg, so no d_first makes it read past the segment arrays.  d_seg_crc is
 * the caller's workspace of nseg uint32 (not overlapping d_crc), left holding
 * each segment's own CRC (what lnx_crc32_segments gives).  nseg == 0 with
 * nframes > 0 is valid (every frame empty); d_bytes, d_start, d_len and
 * d_seg_crc may then be NULL.  Two launches: lnx_crc32_segments' into
 * d_seg_crc, then the fold of each frame's (CRC, length) pairs. */
int lnx_crc32_chain_batch(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                          const uint64_t* d_first, uint64_t nframes, const uint32_t* d_seed, uint32_t* d_seg_crc,
                          uint32_t* d_crc, void* stream);

/* FCS verify of frames made of segments (arguments as lnx_crc32_chain_batch):
 * d_ok[f] = 1 iff frame f's total length >= 4 and its CRC (seed 0) is
 * LNX_CRC32_RESIDUE, wherever the 4 FCS bytes fall (also across a segment
 * boundary); a frame with no segments gives 0.  One byte per frame. */
int lnx_fcs_verify_chain_batch(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                               const uint64_t* d_first, uint64_t nframes, uint32_t* d_seg_crc, uint8_t* d_ok,
                               void* stream);

/* Batched TX FCS append: the tail of
 * StackEthernet.Encapsulate with the CRC32Update hook set
 * (internet/stack-ethernet.go:200-214) for every frame
 * d_bytes[d_start[i] : d_start[i] + d_len[i]]: zero-pad to 60 bytes, write
 * LE32(CRC32(padded frame)) after it, d_len[i] = padded length + 4.  Each frame
 * may grow to `capacity` bytes; a frame that would not fit is left untouched
 * with d_status[i] = 6 (lneto.ErrShortBuffer), else d_status[i] = 0.  Frames
 * in any order; their rooms [start, start + capacity) must not overlap.  A
 * workgroup slice in increasing address order takes the pipelined rows
 * (addressed relative to its first frame), any other slice is folded frame by
 * frame from each frame's own start (as lnx_crc32_segments).  The reference's
 * onSend hook (between padding and FCS) has no batch equivalent. */
int lnx_fcs_append_batch(uint8_t* d_bytes, const uint64_t* d_start, uint32_t* d_len, uint64_t n, uint32_t capacity,
                         uint8_t* d_status, void* stream);

/* Batched transmit checksum generate: for every
 * frame d_bytes[d_start[i] : d_start[i] + d_len[i]] — an Ethernet header and
 * the IP packet a stack child just wrote, before padding and FCS — the step
 * encapsulate4 / encapsulate6 and the ICMP clients run after the child
 * (internet/stack-ip4.go:202-228, internet/stack-ip6.go:167-181,
 * ipv4/icmpv4/client.go:210-214, ipv6/icmpv6/client.go:135-148), in place:
 *   IPv4: total length = len - 14; header CRC over the first 20 bytes
 *         (ipv4/frame.go:138-146); TCP CRC with CRCWriteTCPPseudo; UDP length
 *         = n and UDP CRC with CRCWriteUDPPseudo(n) through NeverZeroSum
 *         (crc.go:65-71); ICMP CRC over the message with a zero seed;
 *   IPv6: payload length = len - 54; TCP / UDP / ICMPv6 CRC with
 *         CRCWritePseudo (ipv6/frame.go:104-108), UDP length = n, NeverZeroSum
 *         for UDP.
 * The header length is the frame's own IHL.  d_status[i] = 0 when done (other
 * EtherTypes and IP protocols: nothing, or the IPv4 header CRC / the IPv6
 * payload length only), else the frame is untouched and d_status[i] = 18
 * (lneto.ErrTruncatedFrame: too short for the IP header or for the TCP 20 /
 * UDP 8 / ICMP 8-byte header the step writes) or 15 (ErrInvalidLengthField:
 * IHL < 5, or a length over 16 bits).  Frames must not overlap.  Two
 * launches, one of which works: the generate rows, or for a batch whose mean
 * of 64 sampled lengths is under 896 B lnx_tx_finish_batch's checksum step
 * (the same bytes and status; d_len is not written either way). */
int lnx_tx_checksum_batch(uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t n,
                          uint8_t* d_status, void* stream);

/* The transmit tail in ONE read of each frame: lnx_tx_checksum_batch's
 * checksum step (flags & LNX_TX_CHECKSUM) followed by lnx_fcs_append_batch's
 * padding and FCS (flags & LNX_TX_FCS), over the frames as the stack wrote them
 * (StackEthernet.Encapsulate after encapsulate4 / encapsulate6,
 * internet/stack-ethernet.go:200-214, internet/stack-ip4.go:202-228,
 * internet/stack-ip6.go:167-181).  The CRC is taken over the frame as loaded
 * and corrected for the fields the checksum step writes, so
 * the result equals the two calls in sequence.  d_len[i] is updated; each frame
 * may grow to `capacity` bytes; d_status[i] = the checksum step's status if
 * non-zero (18, 15), else the append's (0, or 6 lneto.ErrShortBuffer with the
 * frame left unpadded).  Frames must not overlap (any order).  The flag values
 * are LNX_TX_CHECKSUM and LNX_TX_FCS (declared with lnx_egress_packets). */
int lnx_tx_finish_batch(uint8_t* d_bytes, const uint64_t* d_start, uint32_t* d_len, uint64_t n, uint32_t capacity,
                        uint32_t flags, uint8_t* d_status, void* stream);

/* FCS verify of received frames that still carry their 4-byte LE FCS:
 * d_ok[i] = 1 iff len_i >= 4 and CRC32(f[:len_i-4]) == LE32(f[len_i-4:]),
 * evaluated as the residue test CRC32(f) == LNX_CRC32_RESIDUE.  This is the
 * check lneto leaves to the PHY (x/netdev/interface.go:34-40) and would do at
 * netdev.Stack.IngressPackets (x/netdev/interface.go:89) — SURVEY.md §8(f).1.
 * d_off as for lnx_crc32_batch: any order; an end offset below its start is an
 * empty frame (d_ok 0), every other frame, overlapping ones included, gets the
 * verdict of its own bytes. */
int lnx_fcs_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n,
                         uint8_t* d_ok, void* stream);

/* Internet checksum of n segments: d_out[i] = CRC791{d_seed[i]}.PayloadSum16(
 * d_bytes[d_off[i] : d_off[i] + d_len[i]])  (crc.go:52-59).  d_seed may be
 * NULL (all-zero seeds).  The seed is the pseudo-header partial sum written by
 * ipv4.Frame.CRCWriteTCPPseudo / CRCWriteUDPPseudo (ipv4/frame.go:154-170) or
 * ipv6.Frame.CRCWritePseudo (ipv6/frame.go:104-108). */
int lnx_sum16_batch(const uint8_t* d_bytes, const uint64_t* d_off, const uint32_t* d_len,
                    const uint32_t* d_seed, uint64_t n, uint16_t* d_out, void* stream);

/* ---- running internet checksums: raw sums, odd phase, frames made of segments ----
 * As every batch entry these are asynchronous on `stream`, never sync, never
 * read device memory on the host, never allocate and retain nothing; they use
 * no scratch.  A zero count returns LNX_OK; a NULL required pointer with a
 * non-zero count LNX_EINVAL. */

/* The raw 32-bit running sum of n segments (lnx_sum_partial; sumWriteEven /
 * WriteEven, crc.go:23-33, and the odd last byte of crc.go:56):
 *   d_sum[i] = lnx_sum_partial(d_seed ? d_seed[i] : 0, d_bytes[d_off[i] : d_off[i] + d_len[i]], d_phase ? d_phase[i] : 0).
 * d_phase holds one byte per segment of which only bit 0 is read (the parity
 * of the segment's offset in its packet); NULL = every segment at an even
 * offset.  Segments may lie in any order and overlap, as for lnx_sum16_batch.
 * d_sum must not overlap d_seed: the host compares the two address ranges and
 * returns LNX_EINVAL if they do.  A running sum over several calls (data that
 * arrives in pieces) ping-pongs two arrays: call k reads as d_seed the array
 * call k-1 wrote and writes the other, with d_phase = the bytes so far & 1.
 * lnx_sum16_batch with d_seed = a raw sum and d_len = 0 is Sum16()
 * (crc.go:46-49) of it: no finish entry is needed.  A payload's raw sum can be
 * kept and reused as the seed of a rewritten header's sum (a retransmit, a
 * rewritten address or port). */
int lnx_sum_partial_batch(const uint8_t* d_bytes, const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_seed,
                          const uint8_t* d_phase, uint64_t n, uint32_t* d_sum, void* stream);

/* Internet checksum of frames made of segments, laid out as for
 * lnx_crc32_chain_batch: frame f is the concatenation, in index order, of
 * segments d_first[f] .. d_first[f+1]-1; segment k is
 * d_bytes[d_start[k] : d_start[k] + d_len[k]]; d_first holds nframes+1 entries;
 * a frame with d_first[f+1] <= d_first[f] has no segments; every segment index
 * is clamped to nseg in the kernel; nseg == 0 with nframes > 0 is valid
 * (d_bytes, d_start, d_len and d_seg_eo may then be NULL).
 *   d_out16[f] = CRC791{d_seed ? d_seed[f] : 0}.PayloadSum16(frame f)   (crc.go:52-59),
 *   d_sum32[f] = the raw 32-bit sum before sum16 (crc.go:17-21): lnx_sum_partial over the frame.
 * Either output may be NULL, not both.  Segments may lie in any address order,
 * overlap and be empty; a segment behind an odd number of bytes of its frame
 * is summed with its bytes' weights swapped.  d_seg_eo is the caller's
 * workspace of 2 * nseg uint32, left holding every segment's sum of even-offset
 * bytes in [0, nseg) and of odd-offset bytes in [nseg, 2 nseg), each mod 2^32;
 * it must not overlap an output (the host compares the ranges: LNX_EINVAL).
 * Two launches: one that reads each segment's bytes once into d_seg_eo, then
 * the fold of each frame's segments (12 bytes read per segment). */
int lnx_sum16_chain_batch(const uint8_t* d_bytes, const uint64_t* d_start, const uint32_t* d_len, uint64_t nseg,
                          const uint64_t* d_first, uint64_t nframes, const uint32_t* d_seed, uint32_t* d_seg_eo,
                          uint16_t* d_out16, uint32_t* d_sum32, void* stream);

/* Batched ethernet.CRC32Search (ethernet/crc.go:28-47), SURVEY.md §8(f).4:
 * d_result[i] = CRC32Search(d_bytes[d_off[i] : d_off[i+1]], d_min_off[i]) —
 * the first off >= max(minOff, 0) with CRC32(capture[:off]) ==
 * LE32(capture[off:off+4]), or -1 (also when the capture is shorter than
 * minOff + 4: the result is -1 for every int64 d_min_off[i] above len - 4, up
 * to 2^63 - 1).  d_min_off may be NULL (all 0).  For PIO captures of unknown
 * frame length (phy/rmii.md:265-271); every prefix CRC of a capture is
 * computed in one parallel scan.  d_off may be in any order: an end offset
 * below its start is an empty capture (-1), every other capture, overlapping
 * ones included, gets the result of its own bytes. */
int lnx_crc32_search_batch(const uint8_t* d_bytes, const uint64_t* d_off, const int64_t* d_min_off, uint64_t n,
                           int64_t* d_result, void* stream);

/* Receive-path checksum verdicts, fused kernels: for
 * every Ethernet frame d_bytes[d_off[i] : d_off[i+1]] (FCS already stripped)
 * d_verdict[i] = the result lneto's receive path reaches at its checksum
 * stage — StackEthernet.Demux size checks (internet/stack-ethernet.go:139-165),
 * then by EtherType demux4 (internet/stack-ip4.go:100-164: ValidateExceptCRC,
 * IPv4 header sum over the first 20 bytes, TCP / UDP sums with pseudo-header)
 * or demux6 (internet/stack-ip6.go:86-138).  0 = all checks passed or none
 * applies (other EtherTypes); otherwise the lneto errGeneric value
 * (errors.go:6-28): 2 ErrPacketDrop (evil bit, only with LNX_VERIFY_EVIL_BIT;
 * an ICMPv4 type other than echo / echo reply, only with LNX_VERIFY_ICMP),
 * 3 ErrBadCRC, 14 ErrInvalidField, 15 ErrInvalidLengthField,
 * 18 ErrTruncatedFrame.  Destination filtering and handler lookup are stack
 * configuration and are taken as accept-all.  With LNX_VERIFY_ICMP, ICMP
 * messages also take their client's Demux checks up to the checksum
 * (ipv4/icmpv4/client.go:89-102, ipv6/icmpv6/client.go:100-115).  Two
 * launches, one of which works: the ingress rows, or for a batch whose mean
 * frame is under 1280 B the receive check's rows without the CRC (the same
 * verdicts; the choice is made on the device from d_off[0] and d_off[n], with
 * a word of the stream's scratch, as lnx_crc32_batch).  d_off may be in any
 * order (the filtered entry too): an end offset below its start is an empty
 * frame with an empty frame's verdict, every other frame, overlapping ones
 * included, gets the verdict of its own bytes. */
int lnx_ingress_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                             uint8_t* d_verdict, void* stream);

/* The stack configuration behind the receive path's ErrPacketDrop checks, so
 * that a frame the stack would not accept gets ErrPacketDrop (2) with the
 * reference's precedence over the checksum verdicts:
 *   StackEthernet.Demux (internet/stack-ethernet.go:146-161): before
 *     ValidateSize, a frame that is neither broadcast nor for `mac` is dropped
 *     unless eth_accept_multicast and the destination's group bit is set
 *     (SetAcceptMulticast, :56-58); after it, an EtherType with no handler
 *     (RegisterEthernet) is dropped;
 *   demux4 (internet/stack-ip4.go:108-119,135-141): with ip4 != 0.0.0.0, a
 *     destination other than ip4 is dropped before ValidateExceptCRC unless
 *     ip4_accept_multicast and it is 224/4 or ip4_accept_broadcast and it is
 *     255.255.255.255 (ipv4/definitions.go:17-36); a protocol with no handler
 *     (bit p of ip4_protocols: byte p / 8, bit p % 8) is dropped after the
 *     header sum and before the TCP / UDP sums;
 *   demux6 (internet/stack-ip6.go:93-111): with ip6 != ::, a destination other
 *     than ip6 is dropped before ValidateSize unless ip6_accept_multicast and
 *     it is ff00::/8 (internal/ip.go:30-38); a next header with no handler is
 *     dropped before the sums.
 * A NULL filter is accept-all (lnx_ingress_verify_batch). */
typedef struct lnx_rx_filter {  /* (EtherTypes must be > 1500: RegisterEthernet, stack-ethernet.go:131-135) */
  uint8_t mac[6];                 /* StackEthernetConfig.MAC */
  uint8_t eth_accept_multicast;   /* StackEthernet.SetAcceptMulticast */
  uint8_t ip4_accept_multicast;   /* stackip4 SetAcceptMulticast / SetAcceptBroadcast */
  uint8_t ip4_accept_broadcast;
  uint8_t ip6_accept_multicast;   /* stackip6 SetAcceptMulticast6 */
  uint8_t ip4[4];                 /* stackip4 address, all zero = accept every destination */
  uint8_t ip6[16];                /* stackip6 address, all zero = accept every destination */
  uint16_t ethertypes[8];         /* EtherTypes with a registered handler */
  uint32_t n_ethertypes;          /* entries of ethertypes in use (<= 8) */
  uint8_t ip4_protocols[32];      /* 256-bit set of IP protocols with a handler on the IPv4 stack */
  uint8_t ip6_protocols[32];      /* the same for the IPv6 stack */
} lnx_rx_filter;
int lnx_ingress_verify_batch_filtered(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                                      const lnx_rx_filter* filter, uint8_t* d_verdict, void* stream);

/* lneto's whole receive check in ONE pass over each frame:
 * for every frame d_bytes[d_off[i] : d_off[i+1]] carrying its 4-byte LE FCS,
 * d_fcs_ok[i] = the FCS test of lnx_fcs_verify_batch and d_verdict[i] = the
 * verdict lnx_ingress_verify_batch_filtered gives the frame without its FCS
 * (flags LNX_VERIFY_EVIL_BIT / LNX_VERIFY_ICMP, filter NULL = accept-all).
 * With LNX_RX_NO_FCS (a device that strips the FCS) no CRC is taken,
 * d_fcs_ok[i] = 1 and the verdict covers the whole frame.  The receive ring
 * runs it for its batches.  d_off may be in any order: an end offset below its
 * start is an empty frame (d_fcs_ok 0 when a CRC is taken, the verdict of an
 * empty frame), every other frame, overlapping ones included, gets the results
 * of its own bytes. */
int lnx_rx_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                        const lnx_rx_filter* filter, uint8_t* d_fcs_ok, uint8_t* d_verdict, void* stream);

/* Receive delivery: the step after the verdict.  Once
 * demux4 / demux6 have passed the transport sum they call the protocol
 * handler's Demux (internet/stack-ip4.go:135-170, internet/stack-ip6.go:107-138);
 * for TCP and UDP that handler is StackPorts.Demux
 * (internet/stack-ports.go:64-84), which
 *   returns io.ErrShortBuffer when the transport header holds no destination
 *     port (:65-67; the library's 6, as lnx_fcs_append),
 *   returns ErrPacketDrop when no node is registered on that port
 *     (handlers.demuxByPort / nodeByPort, internet/definitions.go:108-116,141-152:
 *     the FIRST node with that local port), and
 *   for a TCP SYN without RST / ACK to such a port queues a RST (:70-82), unless
 *     internal.GetIPAddr rejects the version nibble (internal/ip.go:9-27).
 * A delivery record says, per frame, which handler it goes to or why not.
 * Everything after the first call into that handler (TCP state, StackUDPPort's
 * remote checks, DHCP / DNS / NTP) stays on the host. */
#define LNX_H_ETH 0u      /* + index of the EtherType in filter->ethertypes (first match); + 8 with a NULL filter */
#define LNX_H_IP4 16u     /* + IPv4 protocol, other than TCP / UDP */
#define LNX_H_IP6 272u    /* + IPv6 next header, other than TCP / UDP */
#define LNX_H_TCP 528u    /* + index of the port in ports->tcp (first match); + 256 with NULL ports */
#define LNX_H_UDP 800u    /* + index of the port in ports->udp; + 256 with NULL ports */
#define LNX_H_COUNT 1057u /* handler ids are below it; the bucket of the frames not delivered */
#define LNX_H_NONE 0xFFFFu
#define LNX_DLV_RST 1u    /* TCP miss that queues a RST (stack-ports.go:70-82): src_port, dst_port are filled */
#define LNX_DLV_IP6 2u    /* the IP packet is IPv6 */
#define LNX_DLV_FCS 4u    /* not delivered because its FCS is wrong (verdict 3) */
typedef struct lnx_rx_delivery {
  uint32_t ip_end;    /* end of the IP packet within the frame, 0 for non-IP / not reached */
  uint16_t handler;   /* LNX_H_* id, LNX_H_NONE when not delivered */
  uint16_t l4_off;    /* start of the transport header within the frame */
  uint16_t src_port, dst_port;   /* filled whenever the port stage read them, the RST case included */
  uint8_t verdict;    /* 0 delivered, else the errGeneric number (2 drop, 3 bad CRC, 6 short buffer, 18, ...) */
  uint8_t flags;      /* LNX_DLV_* */
  uint16_t zero;
} lnx_rx_delivery;
/* The nodes registered on StackPorts (Register, stack-ports.go:88-97) in
 * registration order, per protocol; the same tables serve IPv4 and IPv6.
 * Duplicates and port 0 are legal entries (first match).  n_* <= 256. */
typedef struct lnx_rx_ports {
  uint16_t tcp[256];
  uint32_t n_tcp;
  uint16_t udp[256];
  uint32_t n_udp;
} lnx_rx_ports;
/* One frame on the host (len bytes, FCS stripped): verdict_in is its receive
 * verdict (lnx_ingress_verdict, or what the batch entries gave), fcs_ok its FCS
 * result (< 0: none).  In order: fcs_ok == 0 -> verdict 3 with LNX_DLV_FCS;
 * verdict_in != 0 -> that verdict; else the handler by EtherType, IP protocol
 * and port as above.  NULL filter: accept-all; NULL ports: every port has a
 * handler (+ 256).  No read depends on verdict_in: a field the rules need at or
 * past len, or an IP packet that ends past len, gives verdict 18; with a filter,
 * an EtherType (other than IPv4 / IPv6) that it lists no handler for gives
 * verdict 2 even under a zero verdict_in (demuxByProto finds no node).  Fields
 * no rule reached are 0.  Returns LNX_OK, or LNX_EINVAL (NULL out, NULL frame with
 * len > 0, a bad filter, n_tcp / n_udp > 256). */
int lnx_rx_deliver(const uint8_t* frame, size_t len, const lnx_rx_filter* filter, const lnx_rx_ports* ports,
                   int fcs_ok, uint8_t verdict_in, lnx_rx_delivery* out);
/* The same for a batch on the device, chained behind lnx_rx_verify_batch /
 * lnx_ingress_verify_batch[_filtered] on the same d_off (any order; an end below
 * its start is an empty frame): frames carry their FCS and the record is that
 * of the first max(len - 4, 0) bytes, unless flags has LNX_RX_NO_FCS (the only
 * flag).  d_fcs_ok may be NULL (no FCS results).  d_rec[i] (16-byte aligned) is
 * frame i's record.
 * Grouping: d_order (n entries) is a permutation of 0..n-1, the frames by
 * ascending handler id, the frames not delivered last (bucket LNX_H_COUNT), in
 * ARRIVAL ORDER within every bucket (the segments of a connection keep their
 * order); d_count[h] (LNX_H_COUNT + 1 entries) is the size of bucket h.  Both
 * NULL: records only, d_ws is not touched; exactly one NULL: LNX_EINVAL.
 * d_ws: lnx_rx_deliver_ws_bytes(n) bytes of the caller's device memory, 4-byte
 * aligned, used by this call alone until its work on `stream` is done (no
 * per-stream scratch of the library is involved).  n >= 2^32: LNX_EINVAL;
 * n == 0: LNX_OK with d_count zeroed.  Asynchronous on `stream`; retains
 * nothing and never synchronises the device.
 * The receive ring runs this step in lnx_rx_ring_ingress_deliver and
 * lnx_ingress_packets_deliver (below), from the same read as its receive check;
 * lnx_rx_ring_ingress and lnx_ingress_packets keep returning fcs_ok / verdict
 * only. */
uint64_t lnx_rx_deliver_ws_bytes(uint64_t n);
int lnx_rx_deliver_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                         const lnx_rx_filter* filter, const lnx_rx_ports* ports, const uint8_t* d_fcs_ok,
                         const uint8_t* d_verdict, lnx_rx_delivery* d_rec, uint32_t* d_order, uint32_t* d_count,
                         void* d_ws, void* stream);

/* The receive check and the delivery records from ONE read of each frame
 * (DESIGN.md §3.18): d_fcs_ok and d_verdict are, byte for byte, what
 * lnx_rx_verify_batch(d_bytes, d_off, n, flags, filter, ...) writes, and d_rec /
 * d_order / d_count what lnx_rx_deliver_batch writes when chained behind it with
 * those two arrays, the same filter and ports and flags & LNX_RX_NO_FCS.  flags:
 * LNX_VERIFY_EVIL_BIT, LNX_VERIFY_ICMP, LNX_RX_NO_FCS.  d_off in any order.  The
 * receive kernel's lane that holds a frame's FCS result and verdict applies the
 * delivery rules to the header bytes it has staged (past them, for IPv4 options,
 * to the frame's own aligned words), so the header lines are read once; the
 * grouping is the three grouping launches of lnx_rx_deliver_batch on the keys
 * that kernel wrote.  d_order and d_count both NULL: records only, d_ws is not
 * touched; exactly one NULL: LNX_EINVAL.  d_ws: lnx_rx_deliver_ws_bytes(n) bytes,
 * as above.  n == 0: LNX_OK with d_count zeroed.  n >= 2^32, NULL d_rec (or
 * d_fcs_ok / d_verdict), a bad filter, n_tcp / n_udp > 256: LNX_EINVAL.
 * Asynchronous on `stream`; retains nothing, never synchronises the device and
 * uses none of the library's per-stream scratch. */
int lnx_rx_verify_deliver_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                                const lnx_rx_filter* filter, const lnx_rx_ports* ports, uint8_t* d_fcs_ok,
                                uint8_t* d_verdict, lnx_rx_delivery* d_rec, uint32_t* d_order, uint32_t* d_count,
                                void* d_ws, void* stream);

/* RST replies for SYNs to closed ports: the other side effect
 * of StackPorts.Demux on a TCP miss (internet/stack-ports.go:70-82).  A frame
 * queues an entry when its delivery record has LNX_DLV_RST and the version
 * nibble of its byte 14 is 4 (RSTQueue.Queue keeps 4-byte addresses only,
 * tcp/rst.go:22-33; an IPv6 SYN gets no RST); the entry becomes the 54 header
 * bytes RSTQueue.Drain, encapsulate4 and StackEthernet.Encapsulate write
 * (tcp/rst.go:38-63, internet/stack-ip4.go:178-231,
 * internet/stack-ethernet.go:170-217), padded to 60 bytes, with LNX_TX_FCS its
 * LE FCS behind them.  RSTQueue's bound of four entries and its last-in
 * first-out drain are NOT restated: the batch entry makes the reply of every
 * queueing frame, in arrival order, up to `cap`, and reports how many it left
 * out. */
typedef struct lnx_rst_cfg {
  uint8_t mac[6];     /* StackEthernet's MAC: the source */
  uint8_t gw_mac[6];  /* its gateway MAC: the destination */
  uint8_t ip4[4];     /* stackip4's address */
  uint32_t flags;     /* LNX_TX_FCS or 0 */
} lnx_rst_cfg;
typedef struct lnx_tcp_rst {  /* rstEntry, tcp/rst.go:12-19 */
  uint8_t remote_addr[4];
  uint16_t remote_port, local_port;
  uint32_t seq, ack;
  uint16_t flags;  /* tcp.Flags; the frame carries flags & 0x1ff */
  uint16_t zero;
} lnx_tcp_rst;

/* The IP IDs of the next n packets of a stack whose ipID is `ip_id`
 * (internet/stack-ip4.go:189-195, internal/prand.go:4-10): out[0] =
 * Prand16((ip_id + 1) ^ ip4_first), out[k] the same step from out[k - 1].
 * After sending m of them the stack's ipID is out[m - 1]. */
void lnx_ip4_id_chain(uint8_t ip4_first, uint16_t ip_id, uint64_t n, uint16_t* out);
/* The entry frame[0 : len] (FCS stripped) queues under its record: 1 with *out
 * written, 0 for none (*out untouched), LNX_EINVAL for a NULL rec or out or a
 * NULL frame with len > 0.  Only len bounds what is read: a record whose
 * l4_off + 8 > len, or len < 30, queues nothing. */
int lnx_rx_rst_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_tcp_rst* out);
/* The reply of one entry with IP ID ip_id: all 64 bytes of out are written
 * (60..63 zero without LNX_TX_FCS), *len = 64 with LNX_TX_FCS, else 60.
 * LNX_EINVAL for a NULL pointer or an unknown bit in cfg->flags. */
int lnx_tcp_rst_frame(const lnx_rst_cfg* cfg, const lnx_tcp_rst* entry, uint16_t ip_id, uint8_t out[64],
                      uint32_t* len);

/* The replies of a batch, chained behind lnx_rx_deliver_batch /
 * lnx_rx_verify_deliver_batch on the same d_off (any order; an end below its
 * start is an empty frame) and d_rec.  flags: LNX_RX_NO_FCS or 0 (frames carry
 * their FCS).  Reply k answers the k-th queueing frame in index order, lies in
 * the 64-byte slot d_reply + 64 k (d_reply 64-byte aligned; the frame's length
 * is 64 with LNX_TX_FCS in cfg->flags, else 60), carries the IP ID d_ip_id[k]
 * (`cap` entries) and d_src[k] = the index of the frame it answers.  d_n[0] =
 * the replies written = min(wanted, cap), d_n[1] = wanted; slots and d_src
 * entries at or past d_n[0] are not touched.  d_ws: lnx_rx_rst_ws_bytes(n)
 * bytes of the caller's device memory, 4-byte aligned.  Three launches, none
 * waiting for another workgroup and no global atomics: every output is a pure
 * function of the inputs.  n == 0: LNX_OK with d_n zeroed (a NULL d_n: nothing
 * to do); cap == 0: d_n alone is written.  LNX_EINVAL: n >= 2^32, a NULL
 * pointer with work to do, an unknown flag bit on either flags word, a
 * misaligned d_reply.  Asynchronous on `stream`; retains nothing, never
 * synchronises the device and uses none of the library's per-stream scratch. */
uint64_t lnx_rx_rst_ws_bytes(uint64_t n);
int lnx_rx_rst_reply_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                           const lnx_rx_delivery* d_rec, const lnx_rst_cfg* cfg, const uint16_t* d_ip_id, uint64_t cap,
                           uint8_t* d_reply, uint32_t* d_src, uint32_t* d_n, void* d_ws, void* stream);
/* The same frames from explicit entries (the RSTs tcp.Listener queues on the
 * host, tcp/listener.go:221,228): reply k = lnx_tcp_rst_frame(cfg, d_entry[k],
 * d_ip_id[k]) in the slot d_reply + 64 k.  n == 0: LNX_OK. */
int lnx_tcp_rst_frames_batch(const lnx_rst_cfg* cfg, const lnx_tcp_rst* d_entry, uint64_t n, const uint16_t* d_ip_id,
                             uint8_t* d_reply, void* stream);

/* Echo replies for ICMPv4 echo requests: the other frame the
 * stack sends back on its own.  icmpv4.Client.Demux stores an echo request's
 * identifier, sequence number, source address and data
 * (ipv4/icmpv4/client.go:111-132) and the next Encapsulate sends them back as an
 * echo reply (client.go:162-176, 209-218).  A frame queues an entry when its
 * delivery record has verdict 0 and handler LNX_H_IP4 + 1, the record's l4_off
 * and ip_end satisfy 34 <= l4_off, l4_off + 9 <= ip_end <= len and
 * ip_end - l4_off - 8 <= 65507, its ICMP type is 8 and the version nibble of its
 * byte 14 is 4 (for another nibble under a stale record the reference would
 * answer to 0.0.0.0: deliberately not restated).  CONTRACT: the records must come
 * from a receive call with LNX_VERIFY_ICMP (lnx_rx_verify_deliver_batch, or
 * lnx_rx_deliver_batch behind such a check): the request's ICMP checksum
 * (client.go:99-102) is the verdict's business, as the FCS is, and the entry does
 * not check it again.  The entry becomes the frame StackEthernet.Encapsulate,
 * encapsulate4 and Client.Encapsulate write (internet/stack-ethernet.go:170-217,
 * internet/stack-ip4.go:178-231): 42 header bytes (IHL 5, the IP ID, don't
 * fragment, TTL 64, type 0, code 0, the request's id and seq, both checksums
 * taken fresh), the request's data, zero padding to 60 bytes and, with
 * LNX_TX_FCS, its LE FCS.  NOT restated: incomingEcho's capacity and
 * ErrExhausted, the response ring's size, one reply per Encapsulate call and the
 * MTU clip of the carrier buffer; the batch entry answers every queueing frame,
 * in arrival order, up to the caller's capacities, and reports what it left out.
 * lnx_rst_cfg is the stack's side of this reply too. */
typedef struct lnx_icmp_echo {
  uint8_t remote_addr[4];
  uint16_t id, seq;
  uint32_t data_off, data_len;  /* the data is frame[data_off : data_off + data_len], 1 <= data_len <= 65507 */
} lnx_icmp_echo;
/* The entry frame[0 : len] (FCS stripped) queues under its record: 1 with *out
 * written, 0 for none (*out untouched), LNX_EINVAL for a NULL rec or out or a
 * NULL frame with len > 0.  Only len bounds what is read. */
int lnx_rx_echo_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_icmp_echo* out);
/* The reply of one entry with IP ID ip_id and the data data[0 : e->data_len]
 * (frame + e->data_off; it must not overlap out): exactly *len bytes of out are
 * written, *len = max(60, 42 + data_len), plus 4 with LNX_TX_FCS.  Returns
 * LNX_OK; 6 (ErrShortBuffer, as lnx_fcs_append) with nothing written when
 * out_cap is smaller than that; LNX_EINVAL for a NULL pointer, an unknown bit in
 * cfg->flags or a data_len outside 1..65507. */
int lnx_icmp_echo_reply_frame(const lnx_rst_cfg* cfg, const lnx_icmp_echo* e, const uint8_t* data, uint16_t ip_id,
                              uint8_t* out, uint32_t out_cap, uint32_t* len);
/* The replies of a batch, chained behind lnx_rx_deliver_batch /
 * lnx_rx_verify_deliver_batch on the same d_off (any order; an end below its
 * start is an empty frame) and d_rec.  flags: LNX_RX_NO_FCS or 0 (frames carry
 * their FCS).  Reply k answers the k-th queueing frame in index order and
 * carries the IP ID d_ip_id[k].  With len_k its length (FCS included under
 * LNX_TX_FCS) it occupies ceil(len_k / 64) whole 64-byte blocks of d_reply
 * (64-byte aligned), starting at 64 x the sum of the earlier replies' blocks:
 * d_start[k] is that byte offset and d_len[k] = len_k, the form
 * lnx_fcs_verify_segments / lnx_tx_finish_batch take; d_src[k] is the index of
 * the frame it answers; every byte of its blocks is written, zero past len_k.
 * Reply k is written iff k < cap and its last block lies below cap_blocks (a
 * prefix of the replies).  d_n[0..3] = {replies written, replies wanted, blocks
 * written, blocks wanted}, the two block counts saturating at 2^32 - 1.  Nothing of d_reply,
 * d_start, d_len or d_src at or past what was written is touched, and no ID
 * past `written` is read.  d_ws: lnx_rx_echo_ws_bytes(n) bytes of the caller's
 * device memory, 8-byte aligned.  Three launches (count, a one-workgroup scan,
 * build), none waiting for another workgroup and no global atomics: every
 * output is a pure function of the inputs.  n == 0: LNX_OK with d_n zeroed (a
 * NULL d_n: nothing to do); cap == 0 or cap_blocks == 0: d_n alone is written.
 * Alignment: d_reply 64 bytes; d_rec 16 (a record is read as one 16-byte load;
 * the delivery entries write it so aligned); d_start and d_ws 8; d_len, d_src
 * and d_n 4; d_ip_id 2.  LNX_EINVAL: n >= 2^32, a NULL pointer with work to do,
 * an unknown flag bit on either flags word, a pointer that is not so aligned
 * (NULL counts as aligned).  Asynchronous on `stream`; retains
 * nothing, never synchronises the device and uses none of the library's
 * per-stream scratch. */
uint64_t lnx_rx_echo_ws_bytes(uint64_t n);
int lnx_rx_echo_reply_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                            const lnx_rx_delivery* d_rec, const lnx_rst_cfg* cfg, const uint16_t* d_ip_id,
                            uint64_t cap, uint64_t cap_blocks, uint8_t* d_reply, uint64_t* d_start,
                            uint32_t* d_len, uint32_t* d_src, uint32_t* d_n, void* d_ws, void* stream);

/* ARP: the third frame the stack sends back on its own, and
 * the one no IPv4 stack works without.  arp.Handler for IPv4 over Ethernet
 * (HardwareType 1, ProtocolType 0x0800, a 6-byte HardwareAddr, a 4-byte
 * ProtocolAddr), registered on StackEthernet at frame offset 0.  A frame reaches
 * it when its delivery record has verdict 0 and a handler LNX_H_ETH ..
 * LNX_H_ETH + 8, len >= 14 and its EtherType is 0x0806.  Handler.Demux
 * (arp/handler.go:160-203) on b = frame[14:len], P = len - 14: P < 28 gives 18
 * (NewFrame, arp/frame.go:17-22); with minLen = 8 + 2 (b[4] + b[5]), P < minLen
 * gives 18 and else minLen > 255 gives 2 (ValidateSize, arp/frame.go:137-146);
 * a hardware type other than 1 / length other than 6, or a protocol type other
 * than 0x0800 / length other than 4, gives 10; op 1 whose target b[24:28] is
 * cfg->ip4 queues a reply entry {hw = b[8:14], ip = b[14:18]}, the sender (any
 * sender: 0.0.0.0, a broadcast or multicast hardware address), op 1 for another
 * address does nothing, op 2 yields a learn record (the sender again; the
 * cache.Lookup that follows is host state), any other op gives 9.  An entry
 * becomes the 42 bytes Handler.Encapsulate, entry.put and
 * StackEthernet.Encapsulate write (handler.go:126-158, cache.go:32-71,
 * internet/stack-ethernet.go:170-217), padded to 60 bytes, with LNX_TX_FCS its LE
 * FCS behind them: destination = the entry's hw (trySetEthernetDst overwrites
 * the gateway MAC with the ARP body's target hardware address), source = our
 * MAC, 0x0806, 00 01 08 00 06 04 00 02, our MAC, our address, the entry's hw,
 * the entry's ip.  A query (StartQuery, op 1): destination ff:ff:ff:ff:ff:ff,
 * bytes 20-21 = 00 01, the entry's hw (zero from StartQuery) at 32-37 as it is.
 * lnx_rst_cfg is the stack's side here too: mac is both the Ethernet source and
 * the ARP sender (the reference configures the two separately; a working stack
 * keeps them equal), gw_mac is not used.  The handler configured for IPv6, the
 * cache's size, eviction and ageing, cache.Lookup and the resolve callback are
 * NOT restated: the batch entry answers every queueing frame and emits every
 * learn record, in arrival order, up to the caller's capacities, reports what
 * it left out, and the host applies the learn records in order. */
typedef struct lnx_arp_entry { uint8_t hw[6]; uint16_t zero; uint8_t ip[4]; } lnx_arp_entry;       /* 12 bytes */
typedef struct lnx_arp_seen  { uint8_t hw[6]; uint16_t zero; uint8_t ip[4]; uint32_t src; } lnx_arp_seen; /* 16 bytes */
/* frame[0 : len] (FCS stripped) under its record: returns 0 nothing (*out
 * untouched), 1 a request for cfg->ip4 (*out = the sender), 2 an ARP reply
 * (*out = the sender); *verdict (may be NULL) = Handler.Demux's error number,
 * 0 when the frame never reaches the handler.  LNX_EINVAL for a NULL rec, out
 * or cfg or a NULL frame with len > 0.  Only len bounds what is read. */
int lnx_rx_arp_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, const lnx_rst_cfg* cfg,
                     lnx_arp_entry* out, uint8_t* verdict);
/* The frame of one entry, op 1 (query) or 2 (reply): all 64 bytes of out are
 * written (60..63 zero without LNX_TX_FCS), *len = 64 with LNX_TX_FCS, else 60.
 * LNX_EINVAL for a NULL pointer, an op other than 1 or 2 or an unknown bit in
 * cfg->flags. */
int lnx_arp_frame(const lnx_rst_cfg* cfg, uint16_t op, const lnx_arp_entry* e, uint8_t out[64], uint32_t* len);
/* A batch, chained behind lnx_rx_deliver_batch / lnx_rx_verify_deliver_batch on
 * the same d_off (any order; an end below its start is an empty frame) and
 * d_rec.  flags: LNX_RX_NO_FCS or 0 (frames carry their FCS).  Reply k answers
 * the k-th request for cfg->ip4 in index order, lies in the 64-byte slot
 * d_reply + 64 k (the frame's length is 64 with LNX_TX_FCS in cfg->flags, else
 * 60) and d_src[k] is the index of the frame it answers; d_seen[j] is the
 * learn record of the j-th ARP reply in index order, src its frame index, zero
 * 0.  d_n[0..3] = {replies written = min(wanted, cap), replies wanted, seen
 * written = min(wanted, cap_seen), seen wanted}; slots and d_src entries at or
 * past d_n[0] and d_seen entries at or past d_n[2] are not touched.  d_seen may
 * be NULL only with cap_seen == 0 (d_n[2] is 0, d_n[3] still reported).  d_ws:
 * lnx_rx_arp_ws_bytes(n) bytes of the caller's device memory.  Three launches
 * (count, a one-workgroup scan of two sums, build), none waiting for another
 * workgroup and no global atomics: every output is a pure function of the
 * inputs.  n == 0: LNX_OK with d_n zeroed (a NULL d_n: nothing to do); both
 * caps 0: d_n alone is written.  Alignment: d_reply 64 bytes; d_rec and d_seen
 * 16 (each is one 16-byte access); d_src, d_n and d_ws 4.  LNX_EINVAL: n >=
 * 2^32, a NULL pointer with work to do, an unknown flag bit on either flags
 * word, a pointer that is not so aligned (NULL counts as aligned).
 * Asynchronous on `stream`; retains nothing, never synchronises the device and
 * uses none of the library's per-stream scratch. */
uint64_t lnx_rx_arp_ws_bytes(uint64_t n);
int lnx_rx_arp_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint32_t flags,
                     const lnx_rx_delivery* d_rec, const lnx_rst_cfg* cfg, uint64_t cap, uint64_t cap_seen,
                     uint8_t* d_reply, uint32_t* d_src, lnx_arp_seen* d_seen, uint32_t* d_n,
                     void* d_ws, void* stream);
/* The same frames from explicit entries, the host's pending queries and
 * replies: frame k = lnx_arp_frame(cfg, d_op[k], d_entry[k]) in the slot
 * d_reply + 64 k (64-byte aligned; d_entry 4, d_op 2).  On the device an op
 * other than 1 or 2 writes an all-zero slot (there is no per-entry status).
 * n == 0: LNX_OK. */
int lnx_arp_frames_batch(const lnx_rst_cfg* cfg, const lnx_arp_entry* d_entry, const uint16_t* d_op, uint64_t n,
                         uint8_t* d_reply, void* stream);

/* pcap's checksum re-verification over a batch: d_status[i] =
 * lnx_pcap_checksums(d_bytes[d_off[i] : d_off[i+1]]) for every Ethernet frame
 * (FCS stripped; an end offset below its start is an empty frame).  Four
 * frames per wave (16-lane rows); every offset order is allowed. */
int lnx_pcap_verify_batch(const uint8_t* d_bytes, const uint64_t* d_off, uint64_t n, uint8_t* d_status,
                          void* stream);

/* Host-memory convenience: copies h_bytes/h_off to the device, runs
 * lnx_crc32_batch, copies the CRCs back, synchronously.  Used to measure the
 * PCIe-inclusive rate.  nbytes is the length of h_bytes; every
 * offset must be <= nbytes. `device` is the HIP device ordinal. */
int lnx_crc32_batch_host(const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_off,
                         uint64_t n, uint32_t* h_crc, int device);

/* Multi-GPU: the frame index range [0, n) is split into ngpu contiguous
 * slices, one host thread per device; device g computes its slice from its own
 * copy of the data: d_bytes_per_gpu[g] / d_off_per_gpu[g] describe that
 * device's frames (offsets local to its buffer), d_crc_per_gpu[g] receives
 * its results.  No collective, no peer traffic. */
int lnx_crc32_batch_multi(int ngpu, const int* devices, const uint8_t* const* d_bytes_per_gpu,
                          const uint64_t* const* d_off_per_gpu, const uint64_t* n_per_gpu,
                          uint32_t* const* d_crc_per_gpu);

/* ======================================================================== *
 * 3. Receive ring: pinned slots + batched FCS verify / ingress verdicts
 *    
 * ======================================================================== */

/* A pool of `nslots` receive slots of `slot_cap` bytes in pinned host memory,
 * modelled on netdev's bufferSelect (x/netdev/buffer.go:25-37: fixed slots, a
 * length per slot), with `depth` device pipeline stages of `batch_slots`
 * slots each (batch_slots * slot_cap < 2 GiB; 0 = nslots).  A producer writes
 * frames straight into the slots (lnx_rx_ring_slots) and their buffer lengths
 * into lnx_rx_ring_lengths.  slot_cap must be a multiple of 4. */
typedef struct lnx_rx_ring lnx_rx_ring;
int lnx_rx_ring_create(int device, uint32_t nslots, uint32_t slot_cap, uint32_t batch_slots, uint32_t depth,
                       lnx_rx_ring** out);
void lnx_rx_ring_destroy(lnx_rx_ring* ring);
/* Pinned slot memory: slot i is bytes [i*slot_cap, (i+1)*slot_cap). */
uint8_t* lnx_rx_ring_slots(lnx_rx_ring* ring);
/* Pinned buffer length per slot (bytes of slot i in use, <= slot_cap). */
uint32_t* lnx_rx_ring_lengths(lnx_rx_ring* ring);

/* The ring's stack configuration for its verdicts (a copy of *filter is
 * kept; NULL = accept-all, the default).  LNX_EINVAL for more than 8 EtherTypes. */
int lnx_rx_ring_set_filter(lnx_rx_ring* ring, const lnx_rx_filter* filter);

/* Batches of fewer than `frames` frames (lnx_rx_ring_ingress counts,
 * lnx_ingress_packets / lnx_egress_packets n) run on the host with the
 * per-frame functions above (lnx_ingress_verdict, lnx_tx_checksum,
 * lnx_fcs_append, the residue test): no kernel launch, no copy.  The default,
 * LNX_HOST_BATCH_DEFAULT, is the measured crossover of the GPU round trip
 * (DESIGN.md §4 "per-call latency"); 0 sends every batch to the GPU. */
#define LNX_HOST_BATCH_DEFAULT 64u
int lnx_rx_ring_set_host_threshold(lnx_rx_ring* ring, uint32_t frames);

/* Where the ring's frames went since it was created (in the spirit of netdev's
 * RunnerStatistics, x/netdev/runner.go:107-140): frames folded on the host
 * below the threshold, frames and batches (one H2D / kernels / D2H round
 * trip each) sent to the GPU. */
typedef struct lnx_rx_ring_counters {
  uint64_t host_frames;
  uint64_t device_frames;
  uint64_t device_batches;
  uint64_t zero_copy_frames;  /* of device_frames: read (and, egress, patched) in place in the slots */
} lnx_rx_ring_counters;
int lnx_rx_ring_stats(lnx_rx_ring* ring, lnx_rx_ring_counters* out);

/* Zero copy (on by default): the ring's slots are mapped into the GPU's
 * address space and the kernels read the frames in place over PCIe, so no host
 * thread copies a frame and only frame bytes cross the link.  This covers
 * lnx_rx_ring_ingress (a batch whose frames fill >= 90 % of their slots still
 * goes up by DMA of whole slots, the faster mover there) and, when every
 * buffer of a batch lies in the ring's slot memory (netdev
 * RunnerConfig.Buffers carved from lnx_rx_ring_slots,
 * x/netdev/runner.go:92-94), lnx_ingress_packets and lnx_egress_packets (whose
 * kernel then patches the frames in place: one read of each frame, stores of
 * the fields, padding and FCS only).  Other buffers are gathered into pinned
 * staging as before.
 * on = 0 selects the copying forms for every batch. */
int lnx_rx_ring_set_zero_copy(lnx_rx_ring* ring, int on);

/* Device delivers frames without their FCS (x/netdev/interface.go:34-40 leaves
 * the FCS to "device or stack"): no FCS check (fcs_ok = 1), verdicts on the
 * whole frame. */
#define LNX_RX_NO_FCS 4u

/* netdev.Stack.IngressPackets (x/netdev/interface.go:82-89;
 * xnet.Netstack.IngressPackets, x/xnet/netstack.go:103-111) for slots
 * [first, first + count): the frame of slot i is slot[offset : len_i] and
 * carries its 4-byte LE FCS (unless LNX_RX_NO_FCS).  fcs_ok[k] = 1 iff that
 * FCS is right (the check lneto leaves to the PHY, x/netdev/interface.go:34-40);
 * verdict[k] = the receive path's checksum-stage verdict of the frame with the
 * FCS stripped, as lnx_ingress_verify_batch_filtered with the ring's filter.
 * Host output arrays of `count` entries (either may be NULL).  Synchronous;
 * internally the slot range is pipelined over the ring's stages (H2D, kernels,
 * D2H on one HIP stream per stage).  A batch whose frames fill less than 90 %
 * of its slots is packed back to back on the host first, so the copy moves the
 * frame bytes and their offsets, not whole slots. */
int lnx_rx_ring_ingress(lnx_rx_ring* ring, uint32_t first, uint32_t count, uint32_t offset, uint32_t flags,
                        uint8_t* fcs_ok, uint8_t* verdict);

/* The same for caller-owned buffers, exactly IngressPackets(bufs, offset):
 * frame k = bufs[k][offset : lens[k]] (lens[k] <= slot_cap).  The frames are
 * gathered back to back into pinned staging (parallel host copies, overlapped
 * with the device work of the previous batch), so PCIe carries the frame bytes
 * plus 8 bytes of offset per frame; nothing is retained after the call. */
int lnx_ingress_packets(lnx_rx_ring* ring, const uint8_t* const* bufs, const uint32_t* lens, uint64_t n,
                        uint32_t offset, uint32_t flags, uint8_t* fcs_ok, uint8_t* verdict);

/* Receive delivery through the ring.  lnx_rx_ring_set_ports
 * gives the ring the StackPorts tables for it (a copy is kept; NULL, the
 * default: every port has a handler, + 256); n_tcp / n_udp > 256: LNX_EINVAL.
 * lnx_rx_ring_ingress_deliver and lnx_ingress_packets_deliver are
 * lnx_rx_ring_ingress and lnx_ingress_packets (the same routing, host threshold,
 * statistics and error behaviour) whose receive check also writes rec[k], frame
 * k's lnx_rx_delivery under the ring's filter and ports, from the same read of
 * the frame: on the zero-copy routes the header lines cross PCIe once.  rec is
 * required (host memory, count / n entries); fcs_ok and verdict may be NULL;
 * order (count / n entries) and count_out (LNX_H_COUNT + 1 entries) are both
 * given or both NULL (exactly one: LNX_EINVAL, nothing written).  They cover
 * the whole call as lnx_rx_deliver_batch's d_order / d_count would: every
 * internal batch is grouped on the device in its stage's pipeline, and the
 * call's order is the stable concatenation of those groups — for every bucket
 * in ascending order, and for the batches in arrival order, the batch's run of
 * that bucket — so arrival order holds within every bucket.  Below the host
 * threshold the records come from lnx_rx_deliver per frame and the groups from
 * a stable counting sort on the host.  The buffers these entries need are
 * allocated by the first of them (or lnx_rx_ring_set_ports) to be called; a
 * ring that never calls them allocates nothing for them. */
int lnx_rx_ring_set_ports(lnx_rx_ring* ring, const lnx_rx_ports* ports);
int lnx_rx_ring_ingress_deliver(lnx_rx_ring* ring, uint32_t first, uint32_t count, uint32_t offset, uint32_t flags,
                                uint8_t* fcs_ok, uint8_t* verdict, lnx_rx_delivery* rec, uint32_t* order,
                                uint32_t* count_out);
int lnx_ingress_packets_deliver(lnx_rx_ring* ring, const uint8_t* const* bufs, const uint32_t* lens, uint64_t n,
                                uint32_t offset, uint32_t flags, uint8_t* fcs_ok, uint8_t* verdict,
                                lnx_rx_delivery* rec, uint32_t* order, uint32_t* count_out);

/* netdev.Stack.EgressPackets(bufs, sizes, offset) (x/netdev/interface.go:85;
 * xnet.Netstack.EgressPackets, x/xnet/netstack.go:87-98) for the device's part
 * of the transmit path: frame k = bufs[k][offset : offset + lens[k]] is what
 * the stack wrote (Ethernet header + IP packet, before padding and FCS).  With
 * LNX_TX_CHECKSUM its length fields and checksums are generated as
 * lnx_tx_checksum_batch does; with LNX_TX_FCS it is padded to 60 bytes and
 * its LE FCS appended as lnx_fcs_append_batch does, within `capacity` bytes
 * (<= the ring's slot_cap).  The frames come back in place, lens[k] = the new
 * length; status[k] (may be NULL) = the checksum step's status if non-zero,
 * else the append's (0, or 6 ErrShortBuffer with the frame unpadded).
 * Synchronous; the batches are pipelined over the ring's stages (gather, H2D,
 * kernels, D2H, scatter), nothing is retained after the call.  Frames travel
 * packed back to back, each with room for its padding and FCS only.  On an
 * error return the frames of batches that completed before the error may
 * already be written back (with their lens and status); the failing batch's
 * and later lens and status are left as they were, and every stage has
 * drained before the call returns.  The failing batch's frames are left as
 * they were too, except under zero copy (lnx_rx_ring_set_zero_copy), where the
 * kernel patches them in place in the slots: they may then already be padded
 * and carry their FCS while their lens are stale.  Zero copy is taken for a
 * batch only when every frame's room [offset, offset + capacity) lies inside
 * one slot and no slot holds two of the batch's frames.  "The batch" is the
 * internal batch of `batch_slots` consecutive frames (frames [k * batch_slots,
 * (k + 1) * batch_slots) of the call), not the call: a batch that is refused
 * takes the copying form (gathered, finished on the device, written back)
 * while the call's other batches may still be patched in place; the results
 * are the same either way.  An argument error (LNX_EINVAL: capacity >
 * slot_cap, lens[k] > capacity, an unknown flag, a NULL buffer with a length
 * or, under LNX_TX_FCS, at all) is found before anything is written: lens,
 * status and the buffers are then left as they were.  lnx_ingress_packets
 * writes results the same way. */
#define LNX_TX_CHECKSUM 1u
#define LNX_TX_FCS 2u
int lnx_egress_packets(lnx_rx_ring* ring, uint8_t* const* bufs, uint32_t* lens, uint64_t n, uint32_t offset,
                       uint32_t capacity, uint32_t flags, uint8_t* status);

/* Number of visible HIP devices (0 when none). */
int lnx_device_count(void);

/* Human-readable description of the last LNX_EHIP failure on this thread. */
const char* lnx_last_error(void);

/* Library build identification (kernel variant, gfx target). */
const char* lnx_version(void);

#ifdef __cplusplus
}
#endif

#endif /* LNETO_AMD_H */
