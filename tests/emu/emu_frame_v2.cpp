/* tests/emu/emu_frame_v2.cpp -- TEST INFRASTRUCTURE ONLY: what SQZF version 2 (stored blocks) adds to the kernels of
 * sqz_amd/csrc/frame.hip and decode.hip -- the ragged range copy, the version-2 flavours of the index and open
 * kernels, the decode kernels' skip mask -- compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h). */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/decode.hip"

extern "C" {
int emu_range_copy(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                   int len_from_dst, const uint32_t* mask, uint32_t n, int pad8, uint64_t size_hint) {
    sqzk::launch_range_copy(src, src_off, dst, dst_off, len_from_dst ? dst_off : src_off, mask, n, pad8 != 0,
                            size_hint, nullptr);
    return 0;
}
/* the encode side's three steps behind the emit kernel: index, checksum of the index, seal */
int emu_frame_index_v2(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n,
                       uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint8_t* frame,
                       uint64_t capacity, uint64_t* copy_bytes, uint64_t* dense_off, uint32_t* stored,
                       uint64_t* frame_bytes, int32_t* status) {
    uint64_t idx_off[2] = {0, 0};
    uint32_t idx_crc = 0;
    sqzk::launch_frame_index_v2(out_bytes, err, crc, n, content_bytes, win_bits, block_bits, frame, capacity,
                                copy_bytes, dense_off, stored, idx_off, frame_bytes, status, nullptr);
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    sqzk::launch_frame_seal(frame, &idx_crc, n, status, nullptr);
    return 0;
}
/* the decode side's first two steps: checksum of the index, open */
int emu_frame_open_v2(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                      uint32_t n_sel, uint64_t* in_off, uint64_t* out_off, uint32_t* stored, int32_t* status) {
    const uint64_t idx_off[2] = {32, 32 + 8 * (uint64_t)n};
    uint32_t idx_crc = 0;
    if (avail < idx_off[1]) { return 7; }
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    sqzk::launch_frame_open_v2(frame, avail, n, content_bytes, first, n_sel, &idx_crc, in_off, out_off, stored,
                               status, nullptr);
    return 0;
}
/* the launcher without a mask on whatever frame it is given: it keeps its meaning, version 1 only */
int emu_frame_open_v1(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                      uint32_t n_sel, uint64_t* in_off, uint64_t* out_off, int32_t* status) {
    const uint64_t idx_off[2] = {32, 32 + 8 * (uint64_t)n};
    uint32_t idx_crc = 0;
    if (avail < idx_off[1]) { return 7; }
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    sqzk::launch_frame_open(frame, avail, n, content_bytes, first, n_sel, &idx_crc, in_off, out_off, status, nullptr);
    return 0;
}
/* a whole decode as the library chains it: open, entropy decode and expansion under the mask, the stored blocks'
 * copy.  tokens: one slot per output byte (+ 64), tok_count / err: n entries */
int emu_frame_decode_v2(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                        uint32_t n_sel, uint64_t* in_off, uint64_t* out_off, uint32_t* stored, int32_t* status,
                        uint8_t* out, uint32_t* tokens, uint32_t* tok_count, int32_t* err, int waves) {
    const int rc = emu_frame_open_v2(frame, avail, n, content_bytes, first, n_sel, in_off, out_off, stored, status);
    if (rc != 0) { return rc; }
    sqzk::launch_entropy_decode(frame, in_off, out_off, tokens, tok_count, err, nullptr, n_sel, 0, waves, nullptr, stored);
    sqzk::launch_lz_expand(tokens, tok_count, out, out_off, n_sel, nullptr, stored);
    sqzk::launch_range_copy(frame, in_off, out, out_off, out_off, stored, n_sel, false, 0, nullptr);
    return 0;
}
/* the decode kernels alone, as emu_decode.cpp drives them, with a skip mask (null = none) */
int emu_decode_skip(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint8_t* out, const uint64_t* out_off,
                    uint32_t* tokens, uint32_t* tok_count, int32_t* err, int waves, const uint32_t* skip) {
    sqzk::launch_entropy_decode(in, in_off, out_off, tokens, tok_count, err, nullptr, n, 0, waves, nullptr, skip);
    sqzk::launch_lz_expand(tokens, tok_count, out, out_off, n, nullptr, skip);
    return 0;
}
}
