/* tests/emu/emu_frame_v3.cpp -- TEST INFRASTRUCTURE ONLY: SQZF version 3 in the device-resident flavour and the
 * ranged read from a resident frame -- the version-3 kernels of the index and open code, the read plan
 * (sqz_amd/csrc/frame.hip) and the decode kernels with a history behind them (decode.hip) -- compiled for the CPU
 * wave emulator (tests/emu/hip/hip_runtime.h) and chained as sqz_amd/csrc/abi.hip chains them. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/decode.hip"

namespace {
/* the checksum of the caller's dictionary as the library gets it: one range {0, D} written by the plan kernel */
uint32_t dict_crc_of(const uint8_t* dict, uint32_t dict_bytes) {
    uint64_t off[2] = {77, 77}, spare[2] = {0, 0};
    uint32_t crc = 0;
    sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, off, spare, nullptr);
    sqzk::launch_crc32_blocks(dict, off, 1, &crc, dict_bytes, nullptr);
    return crc;
}
}

extern "C" {
/* the encode side's steps behind the emit kernel: the dictionary's checksum, index, checksum of the index, seal */
int emu_frame_index_v3(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n,
                       uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                       const uint8_t* dict, uint32_t dict_bytes, uint8_t* frame, uint64_t capacity,
                       uint64_t* copy_bytes, uint64_t* dense_off, uint32_t* stored, uint64_t* frame_bytes,
                       int32_t* status) {
    uint64_t idx_off[2] = {0, 0};
    uint32_t idx_crc = 0;
    const uint32_t dict_crc = dict_crc_of(dict, dict_bytes);
    sqzk::launch_frame_index_v3(out_bytes, err, crc, n, content_bytes, win_bits, block_bits, flags, dict_bytes,
                                &dict_crc, frame, capacity, copy_bytes, dense_off, stored, idx_off, frame_bytes,
                                status, nullptr);
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 8 * (uint64_t)n + 8, nullptr);
    sqzk::launch_frame_seal(frame, &idx_crc, n, status, nullptr, 8);
    return 0;
}
/* the decode side's first steps: checksum of index and record, checksum of the dictionary, open */
int emu_frame_open_v3(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                      uint32_t n_sel, const uint8_t* dict, uint32_t dict_bytes, uint64_t* in_off, uint64_t* out_off,
                      uint32_t* stored, int32_t* status, uint32_t want_bits) {
    uint64_t idx_off[2] = {77, 77}, spare[2] = {0, 0};
    uint32_t idx_crc = 0;
    if (avail < 32 + 8 * (uint64_t)n + 8) { return 7; }
    sqzk::launch_frame_plan(1, 8 * (uint64_t)n + 8, 8 * (uint64_t)n + 8, 0, idx_off, spare, nullptr);
    sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, &idx_crc, 8 * (uint64_t)n + 8, nullptr);
    const uint32_t dict_crc = dict_crc_of(dict, dict_bytes);
    sqzk::launch_frame_open_v3(frame, avail, n, content_bytes, first, n_sel, &idx_crc, dict_bytes, &dict_crc, in_off,
                               out_off, stored, status, nullptr, want_bits);
    return 0;
}
/* the launchers there were, on whatever frame they are given (masked: launch_frame_open_v2, else launch_frame_open) */
int emu_frame_open_old(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                       uint32_t n_sel, uint64_t* in_off, uint64_t* out_off, uint32_t* stored, int32_t* status,
                       uint32_t want_bits) {
    const uint64_t idx_off[2] = {32, 32 + 8 * (uint64_t)n};
    uint32_t idx_crc = 0;
    if (avail < idx_off[1]) { return 7; }
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    if (stored != nullptr) {
        sqzk::launch_frame_open_v2(frame, avail, n, content_bytes, first, n_sel, &idx_crc, in_off, out_off, stored,
                                   status, nullptr, want_bits);
    } else {
        sqzk::launch_frame_open(frame, avail, n, content_bytes, first, n_sel, &idx_crc, in_off, out_off, status, nullptr);
    }
    return 0;
}
/* a whole decode as the library chains it: open, entropy decode with the dictionary's length as history and the
 * expansion with the dictionary, both under the mask, the stored blocks' copy.  tokens: one slot per output byte
 * (+ 64), tok_count / err: n_sel entries */
int emu_frame_decode_v3(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                        uint32_t n_sel, const uint8_t* dict, uint32_t dict_bytes, uint64_t* in_off, uint64_t* out_off,
                        uint32_t* stored, int32_t* status, uint8_t* out, uint32_t* tokens, uint32_t* tok_count,
                        int32_t* err, int waves) {
    const int rc = emu_frame_open_v3(frame, avail, n, content_bytes, first, n_sel, dict, dict_bytes, in_off, out_off,
                                     stored, status, 0);
    if (rc != 0) { return rc; }
    sqzk::launch_entropy_decode(frame, in_off, out_off, tokens, tok_count, err, nullptr, n_sel, 0, waves, nullptr, stored,
                                dict_bytes);
    sqzk::launch_lz_expand(tokens, tok_count, out, out_off, n_sel, nullptr, stored, dict, dict_bytes);
    sqzk::launch_range_copy(frame, in_off, out, out_off, out_off, stored, n_sel, false, 0, nullptr);
    return 0;
}
/* a ranged read as the library chains it: the covering blocks [first, first + n_sel) decoded into `blocks` and
 * verified against the index, then status and work list, then the copy of the range or of nothing.  crc: n_sel
 * + 1 entries (the mask first, as the library's scratch has it, then the checksums); plan: 5 x uint64 */
int emu_frame_read_v3(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t block_bits,
                      uint64_t offset, uint64_t length, const uint8_t* dict, uint32_t dict_bytes, uint64_t* in_off,
                      uint64_t* out_off, uint32_t* crc, int32_t* status, uint8_t* blocks, uint32_t* tokens,
                      uint32_t* tok_count, int32_t* err, uint64_t* plan, uint8_t* out, int waves) {
    const uint32_t first = (uint32_t)(offset >> block_bits);
    const uint32_t n_sel = (uint32_t)(((offset + length - 1) >> block_bits) + 1) - first;
    const int rc = emu_frame_open_v3(frame, avail, n, content_bytes, first, n_sel, dict, dict_bytes, in_off, out_off,
                                     crc, status, block_bits);
    if (rc != 0) { return rc; }
    sqzk::launch_entropy_decode(frame, in_off, out_off, tokens, tok_count, err, nullptr, n_sel, 0, waves, nullptr, crc,
                                dict_bytes);
    sqzk::launch_lz_expand(tokens, tok_count, blocks, out_off, n_sel, nullptr, crc, dict, dict_bytes);
    sqzk::launch_range_copy(frame, in_off, blocks, out_off, out_off, crc, n_sel, false, 1ull << block_bits, nullptr);
    sqzk::launch_crc32_blocks(blocks, out_off, n_sel, crc, 1ull << block_bits, nullptr);
    sqzk::launch_frame_verify(frame, first, n_sel, crc, status, err, nullptr);
    sqzk::launch_frame_read_plan(err, n_sel, offset - ((uint64_t)first << block_bits), length, plan, status, nullptr);
    sqzk::launch_range_copy(blocks, plan, out, plan + 2, plan + 2, (const uint32_t*)(plan + 4), 1, false, length, nullptr);
    return 0;
}
/* a ranged read's last two steps: status and work list, then the copy kernel.  plan: 5 x uint64 */
int emu_frame_read_plan(const int32_t* err, uint32_t n_sel, uint64_t src_at, uint64_t length, const uint8_t* blocks,
                        uint8_t* out, uint64_t* plan, int32_t* status) {
    sqzk::launch_frame_read_plan(err, n_sel, src_at, length, plan, status, nullptr);
    sqzk::launch_range_copy(blocks, plan, out, plan + 2, plan + 2, (const uint32_t*)(plan + 4), 1, false, length, nullptr);
    return 0;
}
}
