/* tests/emu/emu_frame_gather.cpp -- TEST INFRASTRUCTURE ONLY: many ranges of a resident frame in one call -- the
 * mark, select, plan and copy kernels and the list flavour of the open code (sqz_amd/csrc/frame.hip) with the decode
 * kernels behind them (decode.hip) -- compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h) and chained
 * as sqz_amd/csrc/abi.hip chains them. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/decode.hip"

namespace {
/* the arrays of a call's scratch, each the caller's own allocation so that each can have its guard */
enum { A_BITMAP, A_WPRE, A_CTL, A_SEL, A_IN_OFF, A_OUT_OFF, A_SKIP, A_STORED, A_CRC, A_ERR, A_SRC_OFF, A_MASK,
       A_TOKENS, A_COUNTS, A_BLOCKS, A_N };

void open_list(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, const uint8_t* dict,
               uint32_t dict_bytes, const uint32_t* bitmap, const uint32_t* wpre, const uint32_t* sel,
               const uint32_t* ctl, uint32_t max_blocks, uint64_t* in_off, uint64_t* out_off, uint32_t* skip,
               uint32_t* stored, int32_t* status, uint32_t* blocks_decoded, uint32_t want_bits) {
    const uint64_t idx_bytes = 8 * (uint64_t)n + (dict != nullptr ? 8 : 0);
    uint64_t idx_off[2] = {77, 77}, spare[2] = {0, 0}, dict_off[2] = {77, 77};
    uint32_t idx_crc = 0, dict_crc = 0;
    sqzk::launch_frame_plan(1, idx_bytes, idx_bytes, 0, idx_off, spare, nullptr);
    sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, &idx_crc, idx_bytes, nullptr);
    if (dict != nullptr) {
        sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, dict_off, spare, nullptr);
        sqzk::launch_crc32_blocks(dict, dict_off, 1, &dict_crc, dict_bytes, nullptr);
    }
    sqzk::launch_frame_open_list(frame, avail, n, content_bytes, &idx_crc, dict_bytes, dict != nullptr ? &dict_crc : nullptr,
                                 bitmap, wpre, sel, ctl, max_blocks, in_off, out_off, skip, stored, status,
                                 blocks_decoded, nullptr, want_bits);
}
}

extern "C" {
int emu_gather_mark(const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                    uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks, uint32_t* bitmap) {
    sqzk::launch_gather_mark(offset, length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, nullptr);
    return 0;
}
int emu_gather_select(const uint32_t* bitmap, uint32_t n_blocks, const uint64_t* offset, const uint64_t* length,
                      uint32_t n_ranges, uint64_t max_length, uint64_t content_bytes, uint32_t max_blocks,
                      uint64_t out_capacity, uint32_t* wpre, uint32_t* sel, uint64_t* out_off, uint32_t* ctl) {
    sqzk::launch_gather_select(bitmap, n_blocks, offset, length, n_ranges, max_length, content_bytes, max_blocks,
                               out_capacity, wpre, sel, out_off, ctl, nullptr);
    return 0;
}
/* checksums of index (and record) and dictionary, then the open for a list; dict == NULL: versions 1 and 2 */
int emu_gather_open(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, const uint8_t* dict,
                    uint32_t dict_bytes, const uint32_t* bitmap, const uint32_t* wpre, const uint32_t* sel,
                    const uint32_t* ctl, uint32_t max_blocks, uint64_t* in_off, uint64_t* out_off, uint32_t* skip,
                    uint32_t* stored, int32_t* status, uint32_t* blocks_decoded, uint32_t want_bits) {
    if (avail < 32 + 8 * (uint64_t)n + (dict != nullptr ? 8 : 0)) { return 7; }
    open_list(frame, avail, n, content_bytes, dict, dict_bytes, bitmap, wpre, sel, ctl, max_blocks, in_off, out_off,
              skip, stored, status, blocks_decoded, want_bits);
    return 0;
}
int emu_gather_plan(const uint8_t* frame, const uint64_t* offset, const uint64_t* length, uint32_t n_ranges,
                    uint64_t max_length, uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks,
                    const uint32_t* bitmap, const uint32_t* wpre, const int32_t* err, const uint32_t* crc,
                    const int32_t* status, int32_t* range_err, uint64_t* src_off, uint32_t* mask) {
    sqzk::launch_gather_plan(frame, offset, length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap,
                             wpre, err, crc, status, range_err, src_off, mask, nullptr);
    return 0;
}
/* one work list through either copy kernel: wide != 0 is range_copy_kernel (a workgroup per range), which the
 * library launches with max_length as its size hint */
int emu_gather_copy(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                    const uint64_t* len_off, const uint32_t* mask, uint32_t n_ranges, int wide, uint64_t max_length) {
    if (wide != 0) {
        sqzk::launch_range_copy(src, src_off, dst, dst_off, len_off, mask, n_ranges, false, max_length, nullptr);
    } else {
        sqzk::launch_gather_copy(src, src_off, dst, dst_off, len_off, mask, n_ranges, nullptr);
    }
    return 0;
}
/* the whole call as the library chains it.  a: the A_N arrays above -- bitmap / wpre: ceil(n / 32) (+ 1) words, ctl 2,
 * sel max_blocks, in_off / out_off 2 max_blocks + 1, skip / stored / crc / err / counts 2 max_blocks, src_off / mask
 * n_ranges, tokens (max_blocks << block_bits) + 64, blocks max_blocks << block_bits */
int emu_frame_gather(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t block_bits,
                     const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                     uint32_t max_blocks, const uint8_t* dict, uint32_t dict_bytes, uint8_t* out, uint64_t out_capacity,
                     uint64_t* d_out_off, int32_t* range_err, uint32_t* blocks_decoded, int32_t* status, void** a,
                     int waves, int wide_copy) {
    uint32_t* bitmap = (uint32_t*)a[A_BITMAP]; uint32_t* wpre = (uint32_t*)a[A_WPRE]; uint32_t* ctl = (uint32_t*)a[A_CTL];
    uint32_t* sel = (uint32_t*)a[A_SEL]; uint64_t* in_off = (uint64_t*)a[A_IN_OFF]; uint64_t* out_off = (uint64_t*)a[A_OUT_OFF];
    uint32_t* skip = (uint32_t*)a[A_SKIP]; uint32_t* stored = (uint32_t*)a[A_STORED]; uint32_t* crc = (uint32_t*)a[A_CRC];
    int32_t* err = (int32_t*)a[A_ERR]; uint64_t* src_off = (uint64_t*)a[A_SRC_OFF]; uint32_t* mask = (uint32_t*)a[A_MASK];
    uint32_t* tokens = (uint32_t*)a[A_TOKENS]; uint32_t* counts = (uint32_t*)a[A_COUNTS]; uint8_t* blocks = (uint8_t*)a[A_BLOCKS];
    if (avail < 32 + 8 * (uint64_t)n + (dict != nullptr ? 8 : 0)) { return 7; }
    const uint32_t m = max_blocks < n ? max_blocks : n;
    sqzk::launch_gather_mark(offset, length, n_ranges, max_length, content_bytes, block_bits, n, bitmap, nullptr);
    sqzk::launch_gather_select(bitmap, n, offset, length, n_ranges, max_length, content_bytes, m, out_capacity, wpre,
                               sel, d_out_off, ctl, nullptr);
    open_list(frame, avail, n, content_bytes, dict, dict_bytes, bitmap, wpre, sel, ctl, m, in_off, out_off, skip, stored,
              status, blocks_decoded, block_bits);
    if (m > 0 && n_ranges > 0) {
        sqzk::launch_entropy_decode(frame, in_off, out_off, tokens, counts, err, nullptr, 2 * m, 0, waves, nullptr, skip,
                                    dict_bytes);
        sqzk::launch_lz_expand(tokens, counts, blocks, out_off, 2 * m, nullptr, skip, dict, dict_bytes);
        sqzk::launch_range_copy(frame, in_off, blocks, out_off, out_off, stored, 2 * m, false, 1ull << block_bits, nullptr);
        sqzk::launch_crc32_blocks(blocks, out_off, 2 * m, crc, 1ull << block_bits, nullptr);
    }
    sqzk::launch_gather_plan(frame, offset, length, n_ranges, max_length, content_bytes, block_bits, n, bitmap, wpre, err,
                             crc, status, range_err, src_off, mask, nullptr);
    if (m > 0 && n_ranges > 0) {
        if (wide_copy != 0) {
            sqzk::launch_range_copy(blocks, src_off, out, d_out_off, d_out_off, mask, n_ranges, false, max_length, nullptr);
        } else {
            sqzk::launch_gather_copy(blocks, src_off, out, d_out_off, d_out_off, mask, n_ranges, nullptr);
        }
    }
    return 0;
}
}
