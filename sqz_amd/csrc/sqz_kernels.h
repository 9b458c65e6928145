// sqz_amd/csrc/sqz_kernels.h -- host-visible launchers of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sqz/sqz.h"      // sqz_block_stats

namespace sqzk {

// stage 1: LZ77 brute-force longest-match scan + greedy parse
// (attic/map_experiment/squeeze.h:338-358, :377-394).  Block b reads
// in[in_off[b] .. in_off[b+1]) and writes its token words at
// tokens + in_off[b]; the count goes to tok_count[b].
// waves_per_stream: 1, 2, 4 (default) or 8 wavefronts share one stream's window.
// slots: how many uint32 slots the per-byte arrays (tokens, buf_a, buf_b, match) hold; a block
// whose in_off[b+1] lies beyond them is refused (tok_count[b] = kRefused -> EINVAL in stage 2)
// instead of being written out of bounds.
void launch_lz77_scan(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                      uint32_t window, uint32_t* tokens, uint32_t* tok_count,
                      int waves_per_stream, uint64_t slots, hipStream_t stream);

// stage 1, indexed form: same tokens as launch_lz77_scan without visiting every
// distance (lz77_index.hip): sort -> match -> parse.  buf_a / buf_b / match: one
// uint32 slot per input byte each, addressed like `tokens`.
void launch_index_sort(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                       uint32_t* buf_a, uint32_t* buf_b, uint64_t slots,
                       hipStream_t stream);
void launch_index_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                        uint32_t window, const uint32_t* sorted, uint32_t* match,
                        uint32_t match_groups, uint64_t slots, hipStream_t stream);
void launch_index_parse(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                        const uint32_t* match, uint32_t* tokens, uint32_t* tok_count,
                        uint64_t slots, hipStream_t stream);
// shared dictionary (SQZF version 3), between launch_index_match and either parse: the longest match whose source
// starts in dict[0 .. dict_bytes), 1 <= dict_bytes <= 32767, merged into `match` where it is strictly longer.
// dict_sorted: launch_index_sort's result for the dictionary as a one-block batch.
void launch_dict_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, uint32_t window,
                       const uint8_t* dict, uint32_t dict_bytes, const uint32_t* dict_sorted,
                       uint32_t* match, uint64_t slots, hipStream_t stream);
// the one-step lazy parse over the same match table (not the reference's token sequence; any decoder reads it)
void launch_index_parse_lazy(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                             const uint32_t* match, uint32_t* tokens, uint32_t* tok_count,
                             uint64_t slots, hipStream_t stream);

// stage 2: adaptive-Huffman emit (squeeze.h:278-315, huffman.h, bitstream.h)
void launch_huffman_emit(const uint32_t* tokens, const uint64_t* tok_off,
                         const uint32_t* tok_count, uint8_t* out,
                         const uint64_t* out_off, uint64_t* out_bytes,
                         int32_t* err, uint32_t n_blocks,
                         uint64_t prefix_acc, int prefix_fill, sqz_block_stats* stats,
                         hipStream_t stream);

// test entry: one tree driven by a symbol sequence, its LDS image dumped (huffman_emit.hip)
void launch_tree_debug(const int32_t* symbols, uint32_t count, int which, int batch, uint32_t* dump,
                       hipStream_t stream);

// decode (squeeze.h:502-551): entropy stage -> token words -> LZ77 expansion.
// tokens: one uint32 slot per OUTPUT byte, addressed by out_off; tok_count[n].
// skip (optional, n_blocks entries): a block whose entry is non-zero is not a stream (an SQZF stored block): its
// workgroup leaves at once with err = 0 and tok_count = 0, and the expansion does not touch its output.
void launch_entropy_decode(const uint8_t* in, const uint64_t* in_off, const uint64_t* out_off,
                           uint32_t* tokens, uint32_t* tok_count, int32_t* err, uint64_t* end_bit,
                           uint32_t n_blocks, uint64_t start_bit, int waves, hipStream_t stream,
                           const uint32_t* skip = nullptr, uint32_t history = 0);
// history / dict: every block is preceded by the same `history` = dict_bytes dictionary bytes, which distances may
// reach into (the entropy stage refuses dist > position + history; 0 is a batch without a dictionary)
void launch_lz_expand(const uint32_t* tokens, const uint32_t* tok_count, uint8_t* out,
                      const uint64_t* out_off, uint32_t n_blocks, hipStream_t stream,
                      const uint32_t* skip = nullptr, const uint8_t* dict = nullptr, uint32_t dict_bytes = 0);

// the reference's HEAD range coder (range_coder.hip): literal-only encode as HEAD
// runs it, decode as written.  Block b: in[in_off[b] .. in_off[b+1]) -> out + out_off[b], at most
// out_off[b+1] - out_off[b] bytes; sizes to out_bytes[b], errno (EINVAL/EILSEQ/ERANGE/ENOBUFS) to err[b].
void launch_rc_encode(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                      uint64_t* out_bytes, int32_t* err, uint32_t n_blocks, hipStream_t stream);
void launch_rc_decode(const uint8_t* in, const uint64_t* in_off, uint8_t* out, const uint64_t* out_off,
                      uint64_t* out_bytes, uint64_t* consumed, int32_t* err, uint32_t n_blocks, int dry_error,
                      hipStream_t stream);

// slabs -> dense image of a batch's streams (blocks.hip): block b moves from src + src_off[b]
// to dst + dst_off[b].  bytes[b] and all offsets are multiples of 8.
void launch_compact_blocks(const uint8_t* src, const uint64_t* src_off, const uint64_t* bytes,
                           uint32_t n_blocks, uint8_t* dst, const uint64_t* dst_off,
                           uint64_t avg_bytes, hipStream_t stream);

// the SQZF frame container (frame.hip; format in include/sqz/sqz.h).
// crc[b] = zlib.crc32(in[off[b] .. off[b+1])) for n ranges at arbitrary byte offsets; size_hint = the
// largest range's size when the host knows it (0 = unknown): it only sizes the launch.
void launch_crc32_blocks(const uint8_t* in, const uint64_t* off, uint32_t n_ranges, uint32_t* crc,
                         uint64_t size_hint, hipStream_t stream);
// in_off[k] = min(k * block_bytes, content_bytes), slab_off[k] = k * slab_bytes, k = 0..n_blocks
void launch_frame_plan(uint32_t n_blocks, uint64_t block_bytes, uint64_t content_bytes, uint64_t slab_bytes,
                       uint64_t* in_off, uint64_t* slab_off, hipStream_t stream);
// encode: scan of the stream sizes -> header, index, padding, dense offsets (absolute in the frame),
// frame size and status; then the index checksum into the header
void launch_frame_index(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                        uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint8_t* frame,
                        uint64_t capacity, uint64_t* copy_bytes, uint64_t* dense_off, uint64_t* idx_off,
                        uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream);
// (record_bytes: 8 for a version-3 frame, whose index checksum covers the dictionary's record as well)
void launch_frame_seal(uint8_t* frame, const uint32_t* idx_crc, uint32_t n_blocks, const int32_t* status,
                       hipStream_t stream, uint32_t record_bytes = 0);
// decode: header and index checks, offsets of blocks [first, first + n_sel) for the decode kernels
void launch_frame_open(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                       uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint64_t* in_off,
                       uint64_t* out_off, int32_t* status_out, hipStream_t stream);
// version 2 (SQZ_FRAME_STORED): the same kernels deciding / reading which blocks are stored.  index: stored[n]
// marks them and copy_bytes[] is 0 for them; open: stored[n_sel] is the mask for the decode kernels' `skip`
// and for launch_range_copy (all zeros for a version-1 frame, which this launcher takes as well)
void launch_frame_index_v2(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                           uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint8_t* frame,
                           uint64_t capacity, uint64_t* copy_bytes, uint64_t* dense_off, uint32_t* stored,
                           uint64_t* idx_off, uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream);
void launch_frame_open_v2(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                          uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint64_t* in_off,
                          uint64_t* out_off, uint32_t* stored, int32_t* status_out, hipStream_t stream,
                          uint32_t want_bits = 0);
// ragged copy: len_off[b+1] - len_off[b] bytes from src + src_off[b] to dst + dst_off[b] where mask[b] != 0
// (null: everywhere), any alignment; pad8: zeros up to the next multiple of 8 behind each range.  size_hint
// as for launch_crc32_blocks
void launch_range_copy(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                       const uint64_t* len_off, const uint32_t* mask, uint32_t n_ranges, bool pad8,
                       uint64_t size_hint, hipStream_t stream);
// version 3 (SQZ_FRAME_DICT, with or without SQZ_FRAME_STORED in `flags`): kernels of their own over the same code.
// index: the record { dict_bytes, *dict_crc } behind the entries, idx_off = {32, 32 + 8n + 8}; launch_frame_seal then
// takes record_bytes = 8.  open: idx_crc covers frame[32, 32 + 8n + 8); only a version-3 frame whose record is
// (dict_bytes, *dict_crc) passes (EILSEQ otherwise; EINVAL for versions 1 and 2).  dict_crc: a device pointer to the
// CRC-32 of the caller's dictionary, written by launch_crc32_blocks earlier on the stream.  stored: as for _v2,
// needed for n_sel > 0 (index: only with SQZ_FRAME_STORED).  want_bits (open, _v2 as well): when not 0, a frame
// whose block_bits is another is EINVAL -- for a caller that worked `first` and `n_sel` out from a block_bits
void launch_frame_index_v3(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                           uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                           uint32_t dict_bytes, const uint32_t* dict_crc, uint8_t* frame, uint64_t capacity,
                           uint64_t* copy_bytes, uint64_t* dense_off, uint32_t* stored, uint64_t* idx_off,
                           uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream);
void launch_frame_open_v3(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                          uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint32_t dict_bytes,
                          const uint32_t* dict_crc, uint64_t* in_off, uint64_t* out_off, uint32_t* stored,
                          int32_t* status_out, hipStream_t stream, uint32_t want_bits = 0);
// version 4 (SQZ_FRAME_SHUFFLE, with or without SQZ_FRAME_STORED in `flags`): kernels of their own over the same code.
// index: the record { elem_bytes, 0 } behind the entries, idx_off = {32, 32 + 8n + 8}; launch_frame_seal takes
// record_bytes = 8.  open: idx_crc covers frame[32, 32 + 8n + 8); only a version-4 frame passes (EINVAL for versions
// 1 to 3), and once index_crc has held its record must be { 2 | 4 | 8, 0 } and its first word the caller's
// elem_bytes (EINVAL).  stored, want_bits: as for _v3
void launch_frame_index_v4(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                           uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                           uint32_t elem_bytes, uint8_t* frame, uint64_t capacity, uint64_t* copy_bytes,
                           uint64_t* dense_off, uint32_t* stored, uint64_t* idx_off, uint64_t* frame_bytes_out,
                           int32_t* status_out, hipStream_t stream);
void launch_frame_open_v4(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                          uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint32_t elem_bytes,
                          uint64_t* in_off, uint64_t* out_off, uint32_t* stored, int32_t* status_out,
                          hipStream_t stream, uint32_t want_bits = 0);
// the byte shuffle of version 4 (shuffle.hip): range b = [off[b], off[b + 1]) of src and of dst alike; forward
// dst[j * m + i] = src[i * e + j] with e = elem_bytes (2, 4 or 8; anything else launches nothing) and m = length / e,
// the length % e tail bytes copied; inverse the other way.  Any alignment; src and dst must not overlap; ranges
// with skip[b] != 0 are left alone (null: none).  size_hint as for launch_crc32_blocks
void launch_shuffle_blocks(const uint8_t* src, const uint64_t* off, uint32_t n_ranges, uint32_t elem_bytes,
                           bool inverse, uint8_t* dst, const uint32_t* skip, uint64_t size_hint, hipStream_t stream);
// the same for ranges of mixed element size in one launch: elem[b] = 2, 4 or 8 is launch_shuffle_blocks' transform of
// range b with that element size, 0 copies the range as it is (same row rules, same alignment freedom); any other
// value, like skip[b] != 0, leaves the range alone
void launch_shuffle_ranges(const uint8_t* src, const uint64_t* off, const uint32_t* elem, uint32_t n_ranges,
                           bool inverse, uint8_t* dst, const uint32_t* skip, uint64_t size_hint, hipStream_t stream);
// a ranged read's last step but one: *status = the frame's status, else the first non-zero err[0 .. n_sel); and the
// one-range work list of launch_range_copy(src, plan, dst, plan + 2, plan + 2, (uint32_t*)(plan + 4), 1, ..):
// `length` bytes from src + src_at to dst, masked out unless *status == 0.  plan: 5 x uint64
void launch_frame_read_plan(const int32_t* err, uint32_t n_sel, uint64_t src_at, uint64_t length, uint64_t* plan,
                            int32_t* status, hipStream_t stream);
void launch_frame_verify(const uint8_t* frame, uint32_t first, uint32_t n_sel, const uint32_t* crc,
                         const int32_t* status, int32_t* err, hipStream_t stream);

// many ranges of a resident frame in one call (frame.hip, "gather").  offset / length:
// n_ranges device values each; a range is valid iff length <= max_length, offset <= content_bytes and
// length <= content_bytes - offset.
// mark: zeroes bitmap (ceil(n_blocks / 32) words) and sets the bits of the valid ranges' covering blocks.
// select: wpre (words + 1 entries), sel (max_blocks entries, ascending), out_off (n_ranges + 1: the prefix sum of the
//   valid lengths), ctl[0] = the distinct blocks, ctl[1] = ENOBUFS / ENOSPC / 0 (ctl: 2 words).
// open_list: the checks of launch_frame_open_v2 (dict_crc == nullptr) or launch_frame_open_v3, then TWO entries per
//   slot in in_off / out_off (2 max_blocks + 1 entries), skip and stored (2 max_blocks): entry 2k is block sel[k],
//   decoded to [k << block_bits, ..), entry 2k + 1 the skipped gap up to the next selected stream.  *status_out =
//   the frame's status, else ctl[1]; *blocks_decoded = 0 for a refused frame, else ctl[0].
// plan: range_err, and src_off / mask for the copy of range r to dst + out_off[r] (len_off = dst_off = out_off);
//   err / crc: the decode chain's, 2 max_blocks entries.
// gather_copy: launch_range_copy's work list with 16 lanes per range, for many short ranges; never pads.
void launch_gather_mark(const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                        uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks, uint32_t* bitmap,
                        hipStream_t stream);
void launch_gather_select(const uint32_t* bitmap, uint32_t n_blocks, const uint64_t* offset, const uint64_t* length,
                          uint32_t n_ranges, uint64_t max_length, uint64_t content_bytes, uint32_t max_blocks,
                          uint64_t out_capacity, uint32_t* wpre, uint32_t* sel, uint64_t* out_off, uint32_t* ctl,
                          hipStream_t stream);
void launch_frame_open_list(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                            const uint32_t* idx_crc, uint32_t dict_bytes, const uint32_t* dict_crc,
                            const uint32_t* bitmap, const uint32_t* wpre, const uint32_t* sel, const uint32_t* ctl,
                            uint32_t max_blocks, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                            int32_t* status_out, uint32_t* blocks_decoded, hipStream_t stream, uint32_t want_bits);
void launch_gather_plan(const uint8_t* frame, const uint64_t* offset, const uint64_t* length, uint32_t n_ranges,
                        uint64_t max_length, uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks,
                        const uint32_t* bitmap, const uint32_t* wpre, const int32_t* err, const uint32_t* crc,
                        const int32_t* status, int32_t* range_err, uint64_t* src_off, uint32_t* mask,
                        hipStream_t stream);
void launch_gather_copy(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                        const uint64_t* len_off, const uint32_t* mask, uint32_t n_ranges, hipStream_t stream);

// many ranges WRITTEN into a resident frame in one call (frame.hip, "update"): mark and select as
// for a gather (select's out_off is the data's layout, its capacity the data's size), then
// plan: range_err (EINVAL / 0) and the patch copy's work list (src_off into the data, dst_off into the slots, mask;
//   len_off = data_off), flags[0] = any range invalid; then ctl[1] = the verdict on the request in the call's order
//   (EINVAL for a frame whose win_bits is another, with ctl[2] = 1; ERANGE; ENOBUFS; ENODATA) for launch_frame_open_list.
//   ctl: 3 words here.
// verdict: after the decode chain; *status = the open's, else the first failed touched block's errno; with any status
//   mask[] is cleared and enc_in_off (max_blocks + 1 entries) is all zeros, else enc_in_off[k] = k << block_bits up to
//   the count and the end of the last slot behind it; slab_off[k] = k * slab_bytes.
// merge_index: the new frame's header, index, record and padding from the old entries and the encoder's results
//   (out_bytes, enc_err, crc_new: max_blocks entries by slot), *frame_bytes_out, *status (the encoder's errno, E2BIG),
//   idx_off for the index checksum, and the segment table: seg_dst 2 max_blocks + 2 entries, seg_src / seg_len
//   2 max_blocks + 1.  dict: a version-3 frame (the record is carried over).
// splice: the new payload from the table's three sources; most_bytes sizes the launch.
void launch_update_plan(const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                        uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks, const uint32_t* bitmap,
                        const uint32_t* wpre, const uint64_t* data_off, int32_t* range_err, uint64_t* src_off,
                        uint64_t* dst_off, uint32_t* mask, const uint8_t* frame, uint32_t win_bits, uint32_t* flags,
                        uint32_t* ctl, hipStream_t stream);
void launch_update_verdict(const uint8_t* frame, const uint32_t* sel, const uint32_t* ctl, uint32_t max_blocks,
                           const int32_t* err, const uint32_t* crc, uint32_t block_bits, uint64_t content_bytes,
                           uint64_t slab_bytes, uint32_t n_ranges, int32_t* status, uint32_t* blocks_encoded,
                           uint32_t* mask, uint64_t* enc_in_off, uint64_t* slab_off, hipStream_t stream);
void launch_frame_merge_index(const uint8_t* old, uint32_t n_blocks, uint64_t content_bytes, bool dict,
                              const uint32_t* bitmap, const uint32_t* wpre, const uint32_t* ctl, uint32_t max_blocks,
                              const uint64_t* out_bytes, const int32_t* enc_err, const uint32_t* crc_new,
                              uint64_t slab_bytes, uint8_t* frame, uint64_t capacity, uint64_t* seg_dst, uint64_t* seg_src,
                              uint64_t* seg_len, uint64_t* idx_off, uint64_t* frame_bytes_out, int32_t* status,
                              hipStream_t stream);
void launch_frame_splice(const uint8_t* old, const uint8_t* slabs, const uint8_t* slots, uint8_t* dst,
                         const uint64_t* seg_dst, const uint64_t* seg_src, const uint64_t* seg_len, uint32_t max_blocks,
                         uint64_t most_bytes, hipStream_t stream);
// splice over a table of `segments` segments (seg_dst: segments + 1 entries)
void launch_frame_splice_segments(const uint8_t* old, const uint8_t* slabs, const uint8_t* slots, uint8_t* dst,
                                  const uint64_t* seg_dst, const uint64_t* seg_src, const uint64_t* seg_len,
                                  uint32_t segments, uint64_t most_bytes, hipStream_t stream);

// data_bytes more content behind a resident frame in one call (frame.hip, "append").  The host
// knows t = content_bytes mod 2^block_bits, whether the last block is touched (t > 0 and data_bytes > 0), keep =
// n_blocks - (touched ? 1 : 0) and m = ceil((t + data_bytes) / 2^block_bits) (0 for no data).
// plan: bitmap (ceil(n_blocks / 32) words), wpre (words + 1), sel (1 entry) and ctl[0] for launch_frame_open_list with
//   max_blocks = 1 -- the last block iff it is touched -- and ctl[1] = EINVAL for a frame whose win_bits is another
//   (ctl: 2 words).
// verdict: after the decode chain (entry 0 of err / crc is the touched block's); *blocks_encoded = 0 under a status of
//   the open's, else m; *status = the open's, else the touched block's errno or EILSEQ; copy (5 x uint64): the one-range
//   work list launch_range_copy(data, copy, staging, copy + 1, copy + 2, (uint32_t*)(copy + 4), 1, ..) of the data to
//   staging + t, masked out under any status; enc_in_off / slab_off (m + 1 entries): the encoder's blocks over the
//   staging area (all empty under any status) and their slabs.
// append_index: the new frame's header, n' = keep + m entries, record and padding from the old entries and the
//   encoder's results (out_bytes, enc_err, crc_new: m entries), *frame_bytes_out, *status (the encoder's errno, E2BIG),
//   idx_off for the index checksum, and the segment table: seg_dst m + 2 entries, seg_src / seg_len m + 1.
void launch_append_plan(const uint8_t* frame, uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                        uint32_t block_bits, uint32_t win_bits, uint32_t* bitmap, uint32_t* wpre, uint32_t* sel,
                        uint32_t* ctl, hipStream_t stream);
void launch_append_verdict(const uint8_t* frame, uint32_t n_blocks, const uint32_t* ctl, const int32_t* err,
                           const uint32_t* crc, uint32_t block_bits, uint64_t content_bytes, uint64_t data_bytes,
                           uint32_t m, uint64_t slab_bytes, int32_t* status, uint32_t* blocks_encoded, uint64_t* copy,
                           uint64_t* enc_in_off, uint64_t* slab_off, hipStream_t stream);
void launch_frame_append_index(const uint8_t* old, uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                               uint32_t m, bool dict, const uint64_t* out_bytes, const int32_t* enc_err,
                               const uint32_t* crc_new, uint64_t slab_bytes, uint8_t* frame, uint64_t capacity,
                               uint64_t* seg_dst, uint64_t* seg_src, uint64_t* seg_len, uint64_t* idx_off,
                               uint64_t* frame_bytes_out, int32_t* status, hipStream_t stream);

// k frames in one call (frame.hip, "batches of frames"): a workgroup per frame, launches that do
// not depend on k.  base[f] (k + 1 entries) = the blocks in front of frame f.
// encode_scan: from the k sizes in_at (the contents lie back to back), frame_at (the bounds of sqz_frame_bound_ex,
//   each rounded up to 16) and base, k + 1 entries each.
// plan: launch_frame_plan for every frame's blocks at base[f] of in_off / slab_off (total blocks + 1 entries).
// index: launch_frame_index / _v2 for frame f at frames + frame_at[f] over its slice of out_bytes, err, crc, copy_bytes,
//   stored (null without SQZ_FRAME_STORED), frame_bytes_out[f] and status_out[f]; the index checksum and the seal in
//   the same workgroup; dense_off (total blocks + 1) absolute in `frames` for ONE launch_compact_blocks and ONE
//   launch_range_copy over the batch.  dense_rel: total blocks + k entries of room.
// decode_scan: base from items[].n_blocks.
// open: launch_frame_open_v2 (all blocks) for frame f over its n + 1 ENTRIES at base[f] + f of in_off / out_off (total
//   blocks + k + 1 entries; in_off absolute in `frames`, out_off = out_at[f] - out_base + the block's place), skip and
//   stored (total blocks + k); entry n of a frame is switched off and reaches to the next frame's first stream.  The
//   index checksum is taken in the same workgroup.  A refused frame: status_out[f], every entry empty and switched off.
// verify: launch_frame_verify for every frame; err by entry in, err_out by block (at base[f]) out.
void launch_frames_encode_scan(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits, uint32_t flags,
                               uint64_t* in_at, uint64_t* frame_at, uint32_t* base, hipStream_t stream);
void launch_frames_plan(const uint64_t* content_bytes, const uint64_t* in_at, const uint32_t* base, uint32_t k,
                        uint32_t block_bits, uint64_t slab_bytes, uint64_t* in_off, uint64_t* slab_off,
                        hipStream_t stream);
void launch_frames_index(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc,
                         const uint64_t* content_bytes, const uint64_t* frame_at, const uint32_t* base, uint32_t k,
                         uint32_t win_bits, uint32_t block_bits, uint32_t flags, uint8_t* frames, uint64_t* copy_bytes,
                         uint64_t* dense_rel, uint64_t* dense_off, uint32_t* stored, uint64_t* frame_bytes_out,
                         int32_t* status_out, hipStream_t stream);
void launch_frames_decode_scan(const sqz_frames_item* items, uint32_t k, uint32_t* base, hipStream_t stream);
void launch_frames_open(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                        uint64_t out_base, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                        int32_t* status_out, hipStream_t stream);
void launch_frames_verify(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                          const uint32_t* crc, const int32_t* status, const int32_t* err, int32_t* err_out,
                          hipStream_t stream);
// The flavours that know version 4: elem[f] (k words: 0, 2, 4 or 8) is frame f's element size, 0 an unshuffled frame.
// encode_scan_v4: a shuffled frame's bound is sqz_frame_bound_shuf's (the record's 8 bytes in front of the padding).
// plan_v4: in addition blk_elem (total blocks entries) = the element size of every block, for launch_shuffle_ranges.
// index_v4: frame f is launch_frame_index_v4's where elem[f] != 0 (flags bit 2, the record, which the checksum covers).
// open_v4: items[f].zero carries the caller's element size for frame f.  A version-4 header is opened by
//   launch_frame_open_v4 with it (EINVAL when it is 0), a version-1 or -2 header as above (EINVAL when it is not 0),
//   version 3 is EINVAL.  ent_elem (total blocks + k entries): the element size of every entry, 0 for the switched-off
//   one of every frame.  The caller made sure that avail covers the record where the element size is not 0.
void launch_frames_encode_scan_v4(const uint64_t* content_bytes, const uint32_t* elem, uint32_t k, uint32_t block_bits,
                                  uint32_t flags, uint64_t* in_at, uint64_t* frame_at, uint32_t* base,
                                  hipStream_t stream);
void launch_frames_plan_v4(const uint64_t* content_bytes, const uint32_t* elem, const uint64_t* in_at,
                           const uint32_t* base, uint32_t k, uint32_t block_bits, uint64_t slab_bytes, uint64_t* in_off,
                           uint64_t* slab_off, uint32_t* blk_elem, hipStream_t stream);
void launch_frames_index_v4(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc,
                            const uint64_t* content_bytes, const uint32_t* elem, const uint64_t* frame_at,
                            const uint32_t* base, uint32_t k, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                            uint8_t* frames, uint64_t* copy_bytes, uint64_t* dense_rel, uint64_t* dense_off,
                            uint32_t* stored, uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream);
void launch_frames_open_v4(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                           uint64_t out_base, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                           uint32_t* ent_elem, int32_t* status_out, hipStream_t stream);

} // namespace sqzk
