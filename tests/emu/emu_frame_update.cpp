/* tests/emu/emu_frame_update.cpp -- TEST INFRASTRUCTURE ONLY: many ranges written into a resident frame in one call --
 * the plan, verdict, merge-index and splice kernels (sqz_amd/csrc/frame.hip) behind the gather's mark, select and open
 * and the decode kernels (decode.hip) -- compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h) and chained as
 * sqz_amd/csrc/abi.hip chains them.  The encoder does not run here: the caller hands the touched blocks' new streams
 * in as the slabs' contents, with their sizes and errnos. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/decode.hip"

namespace {
/* the arrays of a call's scratch, each the caller's own allocation so that each can have its guard */
enum { A_BITMAP, A_WPRE, A_CTL, A_SEL, A_IN_OFF, A_OUT_OFF, A_SKIP, A_STORED, A_CRC, A_ERR, A_SRC_OFF, A_MASK,
       A_TOKENS, A_COUNTS, A_SLOTS, A_DST_OFF, A_ENC_IN_OFF, A_SLAB_OFF, A_OUT_BYTES, A_ENC_ERR, A_CRC_NEW, A_SEG_DST,
       A_SEG_SRC, A_SEG_LEN, A_FLAGS, A_SLABS, A_N };
}

extern "C" {
uint64_t emu_update_chunk(void) { return sqzk::kSpliceChunk; }

int emu_update_plan(const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                    uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks, const uint32_t* bitmap,
                    const uint32_t* wpre, const uint64_t* data_off, int32_t* range_err, uint64_t* src_off,
                    uint64_t* dst_off, uint32_t* mask, const uint8_t* frame, uint32_t win_bits, uint32_t* flags,
                    uint32_t* ctl) {
    sqzk::launch_update_plan(offset, length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, wpre,
                             data_off, range_err, src_off, dst_off, mask, frame, win_bits, flags, ctl, nullptr);
    return 0;
}
int emu_update_verdict(const uint8_t* frame, const uint32_t* sel, const uint32_t* ctl, uint32_t max_blocks,
                       const int32_t* err, const uint32_t* crc, uint32_t block_bits, uint64_t content_bytes,
                       uint64_t slab_bytes, uint32_t n_ranges, int32_t* status, uint32_t* blocks_encoded, uint32_t* mask,
                       uint64_t* enc_in_off, uint64_t* slab_off) {
    sqzk::launch_update_verdict(frame, sel, ctl, max_blocks, err, crc, block_bits, content_bytes, slab_bytes, n_ranges,
                                status, blocks_encoded, mask, enc_in_off, slab_off, nullptr);
    return 0;
}
int emu_update_merge(const uint8_t* old, uint32_t n_blocks, uint64_t content_bytes, int dict, const uint32_t* bitmap,
                     const uint32_t* wpre, const uint32_t* ctl, uint32_t max_blocks, const uint64_t* out_bytes,
                     const int32_t* enc_err, const uint32_t* crc_new, uint64_t slab_bytes, uint8_t* frame,
                     uint64_t capacity, uint64_t* seg_dst, uint64_t* seg_src, uint64_t* seg_len, uint64_t* idx_off,
                     uint64_t* frame_bytes, int32_t* status) {
    sqzk::launch_frame_merge_index(old, n_blocks, content_bytes, dict != 0, bitmap, wpre, ctl, max_blocks, out_bytes,
                                   enc_err, crc_new, slab_bytes, frame, capacity, seg_dst, seg_src, seg_len, idx_off,
                                   frame_bytes, status, nullptr);
    return 0;
}
int emu_update_splice(const uint8_t* old, const uint8_t* slabs, const uint8_t* slots, uint8_t* dst,
                      const uint64_t* seg_dst, const uint64_t* seg_src, const uint64_t* seg_len, uint32_t max_blocks,
                      uint64_t most_bytes) {
    sqzk::launch_frame_splice(old, slabs, slots, dst, seg_dst, seg_src, seg_len, max_blocks, most_bytes, nullptr);
    return 0;
}
/* the whole call as the library chains it, the encoder's results (A_SLABS, A_OUT_BYTES, A_ENC_ERR: by slot) given.
 * a: the A_N arrays above -- the gather's (ctl 3 words), dst_off n_ranges, enc_in_off / slab_off max_blocks + 1,
 * out_bytes / enc_err / crc_new max_blocks, seg_dst 2 max_blocks + 2, seg_src / seg_len 2 max_blocks + 1, flags 1,
 * slabs max_blocks * slab_bytes */
int emu_frame_update(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t win_bits,
                     uint32_t block_bits, const uint64_t* offset, const uint64_t* length, uint32_t n_ranges,
                     uint64_t max_length, uint32_t max_blocks, const uint8_t* data, uint64_t data_bytes,
                     uint64_t* data_off, const uint8_t* dict, uint32_t dict_bytes, uint8_t* new_frame, uint64_t capacity,
                     uint64_t* frame_bytes, int32_t* range_err, uint32_t* blocks_encoded, int32_t* status, void** a,
                     uint64_t slab_bytes, int wide_copy) {
    uint32_t* bitmap = (uint32_t*)a[A_BITMAP]; uint32_t* wpre = (uint32_t*)a[A_WPRE]; uint32_t* ctl = (uint32_t*)a[A_CTL];
    uint32_t* sel = (uint32_t*)a[A_SEL]; uint64_t* in_off = (uint64_t*)a[A_IN_OFF]; uint64_t* out_off = (uint64_t*)a[A_OUT_OFF];
    uint32_t* skip = (uint32_t*)a[A_SKIP]; uint32_t* stored = (uint32_t*)a[A_STORED]; uint32_t* crc = (uint32_t*)a[A_CRC];
    int32_t* err = (int32_t*)a[A_ERR]; uint64_t* src_off = (uint64_t*)a[A_SRC_OFF]; uint32_t* mask = (uint32_t*)a[A_MASK];
    uint32_t* tokens = (uint32_t*)a[A_TOKENS]; uint32_t* counts = (uint32_t*)a[A_COUNTS]; uint8_t* slots = (uint8_t*)a[A_SLOTS];
    uint64_t* dst_off = (uint64_t*)a[A_DST_OFF]; uint64_t* enc_in_off = (uint64_t*)a[A_ENC_IN_OFF];
    uint64_t* slab_off = (uint64_t*)a[A_SLAB_OFF]; uint64_t* out_bytes = (uint64_t*)a[A_OUT_BYTES];
    int32_t* enc_err = (int32_t*)a[A_ENC_ERR]; uint32_t* crc_new = (uint32_t*)a[A_CRC_NEW];
    uint64_t* seg_dst = (uint64_t*)a[A_SEG_DST]; uint64_t* seg_src = (uint64_t*)a[A_SEG_SRC];
    uint64_t* seg_len = (uint64_t*)a[A_SEG_LEN]; uint32_t* flags = (uint32_t*)a[A_FLAGS]; uint8_t* slabs = (uint8_t*)a[A_SLABS];
    const uint64_t record = dict != nullptr ? 8 : 0;
    if (avail < 32 + 8 * (uint64_t)n + record) { return 7; }
    const uint32_t m = max_blocks < n ? max_blocks : n;
    const uint64_t bb = 1ull << block_bits;
    sqzk::launch_gather_mark(offset, length, n_ranges, max_length, content_bytes, block_bits, n, bitmap, nullptr);
    sqzk::launch_gather_select(bitmap, n, offset, length, n_ranges, max_length, content_bytes, m, data_bytes, wpre, sel,
                               data_off, ctl, nullptr);
    sqzk::launch_update_plan(offset, length, n_ranges, max_length, content_bytes, block_bits, n, bitmap, wpre, data_off,
                             range_err, src_off, dst_off, mask, frame, win_bits, flags, ctl, nullptr);
    const uint64_t idx_bytes = 8 * (uint64_t)n + record;
    uint64_t idx_off[2] = {77, 77}, spare[2] = {0, 0}, dict_off[2] = {77, 77}, new_idx_off[2] = {77, 77};
    uint32_t idx_crc = 0, dict_crc = 0, new_idx_crc = 0;
    sqzk::launch_frame_plan(1, idx_bytes, idx_bytes, 0, idx_off, spare, nullptr);
    sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, &idx_crc, idx_bytes, nullptr);
    if (dict != nullptr) {
        sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, dict_off, spare, nullptr);
        sqzk::launch_crc32_blocks(dict, dict_off, 1, &dict_crc, dict_bytes, nullptr);
    }
    sqzk::launch_frame_open_list(frame, avail, n, content_bytes, &idx_crc, dict_bytes, dict != nullptr ? &dict_crc : nullptr,
                                 bitmap, wpre, sel, ctl, m, in_off, out_off, skip, stored, status, blocks_encoded, nullptr,
                                 block_bits);
    const bool work = m > 0 && n_ranges > 0;
    if (work) {
        sqzk::launch_entropy_decode(frame, in_off, out_off, tokens, counts, err, nullptr, 2 * m, 0, 1, nullptr, skip, dict_bytes);
        sqzk::launch_lz_expand(tokens, counts, slots, out_off, 2 * m, nullptr, skip, dict, dict_bytes);
        sqzk::launch_range_copy(frame, in_off, slots, out_off, out_off, stored, 2 * m, false, bb, nullptr);
        sqzk::launch_crc32_blocks(slots, out_off, 2 * m, crc, bb, nullptr);
    }
    sqzk::launch_update_verdict(frame, sel, ctl, m, err, crc, block_bits, content_bytes, slab_bytes, n_ranges, status,
                                blocks_encoded, mask, enc_in_off, slab_off, nullptr);
    if (work) {
        if (wide_copy != 0) {
            sqzk::launch_range_copy(data, src_off, slots, dst_off, data_off, mask, n_ranges, false, max_length, nullptr);
        } else {
            sqzk::launch_gather_copy(data, src_off, slots, dst_off, data_off, mask, n_ranges, nullptr);
        }
        sqzk::launch_crc32_blocks(slots, enc_in_off, m, crc_new, bb, nullptr);
    }
    sqzk::launch_frame_merge_index(frame, n, content_bytes, dict != nullptr, bitmap, wpre, ctl, m, out_bytes, enc_err,
                                   crc_new, slab_bytes, new_frame, capacity, seg_dst, seg_src, seg_len, new_idx_off,
                                   frame_bytes, status, nullptr);
    sqzk::launch_crc32_blocks(new_frame, new_idx_off, 1, &new_idx_crc, idx_bytes, nullptr);
    sqzk::launch_frame_seal(new_frame, &new_idx_crc, n, status, nullptr, (uint32_t)record);
    const uint64_t payload_off = (32 + idx_bytes + 15) & ~(uint64_t)15;
    sqzk::launch_frame_splice(frame, slabs, slots, new_frame, seg_dst, seg_src, seg_len, m,
                              capacity > payload_off ? capacity - payload_off : 0, nullptr);
    return 0;
}
}
