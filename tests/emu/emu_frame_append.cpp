/* tests/emu/emu_frame_append.cpp -- TEST INFRASTRUCTURE ONLY: more content behind a resident frame in one call -- the
 * plan, verdict and append-index kernels (sqz_amd/csrc/frame.hip) with the open for a list, the decode kernels
 * (decode.hip), the range copy, the checksums, the seal and the splice -- compiled for the CPU wave emulator
 * (tests/emu/hip/hip_runtime.h) and chained as sqz_amd/csrc/abi.hip chains them.  The encoder does not run here: the
 * caller hands the new blocks' streams in as the slabs' contents, with their sizes and errnos. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/decode.hip"

namespace {
/* the arrays of a call's scratch, each the caller's own allocation so that each can have its guard */
enum { A_BITMAP, A_WPRE, A_CTL, A_SEL, A_IN_OFF, A_OUT_OFF, A_SKIP, A_STORED, A_CRC, A_ERR, A_TOKENS, A_COUNTS,
       A_STAGING, A_COPY, A_ENC_IN_OFF, A_SLAB_OFF, A_OUT_BYTES, A_ENC_ERR, A_CRC_NEW, A_SEG_DST, A_SEG_SRC, A_SEG_LEN,
       A_SLABS, A_N };
}

extern "C" {
int emu_append_plan(const uint8_t* frame, uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                    uint32_t block_bits, uint32_t win_bits, uint32_t* bitmap, uint32_t* wpre, uint32_t* sel,
                    uint32_t* ctl) {
    sqzk::launch_append_plan(frame, n_blocks, content_bytes, data_bytes, block_bits, win_bits, bitmap, wpre, sel, ctl,
                             nullptr);
    return 0;
}
int emu_append_verdict(const uint8_t* frame, uint32_t n_blocks, const uint32_t* ctl, const int32_t* err,
                       const uint32_t* crc, uint32_t block_bits, uint64_t content_bytes, uint64_t data_bytes, uint32_t m,
                       uint64_t slab_bytes, int32_t* status, uint32_t* blocks_encoded, uint64_t* copy,
                       uint64_t* enc_in_off, uint64_t* slab_off) {
    sqzk::launch_append_verdict(frame, n_blocks, ctl, err, crc, block_bits, content_bytes, data_bytes, m, slab_bytes,
                                status, blocks_encoded, copy, enc_in_off, slab_off, nullptr);
    return 0;
}
int emu_append_index(const uint8_t* old, uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes, uint32_t m,
                     int dict, const uint64_t* out_bytes, const int32_t* enc_err, const uint32_t* crc_new,
                     uint64_t slab_bytes, uint8_t* frame, uint64_t capacity, uint64_t* seg_dst, uint64_t* seg_src,
                     uint64_t* seg_len, uint64_t* idx_off, uint64_t* frame_bytes, int32_t* status) {
    sqzk::launch_frame_append_index(old, n_blocks, content_bytes, data_bytes, m, dict != 0, out_bytes, enc_err, crc_new,
                                    slab_bytes, frame, capacity, seg_dst, seg_src, seg_len, idx_off, frame_bytes, status,
                                    nullptr);
    return 0;
}
int emu_append_splice(const uint8_t* old, const uint8_t* slabs, const uint8_t* staging, uint8_t* dst,
                      const uint64_t* seg_dst, const uint64_t* seg_src, const uint64_t* seg_len, uint32_t segments,
                      uint64_t most_bytes) {
    sqzk::launch_frame_splice_segments(old, slabs, staging, dst, seg_dst, seg_src, seg_len, segments, most_bytes, nullptr);
    return 0;
}
/* the whole call as the library chains it, the encoder's results (A_SLABS, A_OUT_BYTES, A_ENC_ERR: by new block)
 * given.  a: the A_N arrays above -- bitmap words, wpre words + 1, ctl 2, sel 1, in_off / out_off 3, skip / stored /
 * crc / err 2, staging t + data_bytes + 16, copy 5, enc_in_off / slab_off m + 1, out_bytes / enc_err / crc_new m,
 * seg_dst m + 2, seg_src / seg_len m + 1, slabs m * slab_bytes.  m, n_new, touched: the host's arithmetic. */
int emu_frame_append(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t win_bits,
                     uint32_t block_bits, const uint8_t* data, uint64_t data_bytes, const uint8_t* dict,
                     uint32_t dict_bytes, uint8_t* new_frame, uint64_t capacity, uint64_t* frame_bytes,
                     uint32_t* blocks_encoded, int32_t* status, void** a, uint64_t slab_bytes, uint32_t m,
                     uint32_t n_new, int touched) {
    uint32_t* bitmap = (uint32_t*)a[A_BITMAP]; uint32_t* wpre = (uint32_t*)a[A_WPRE]; uint32_t* ctl = (uint32_t*)a[A_CTL];
    uint32_t* sel = (uint32_t*)a[A_SEL]; uint64_t* in_off = (uint64_t*)a[A_IN_OFF]; uint64_t* out_off = (uint64_t*)a[A_OUT_OFF];
    uint32_t* skip = (uint32_t*)a[A_SKIP]; uint32_t* stored = (uint32_t*)a[A_STORED]; uint32_t* crc = (uint32_t*)a[A_CRC];
    int32_t* err = (int32_t*)a[A_ERR]; uint32_t* tokens = (uint32_t*)a[A_TOKENS]; uint32_t* counts = (uint32_t*)a[A_COUNTS];
    uint8_t* staging = (uint8_t*)a[A_STAGING]; uint64_t* copy = (uint64_t*)a[A_COPY];
    uint64_t* enc_in_off = (uint64_t*)a[A_ENC_IN_OFF]; uint64_t* slab_off = (uint64_t*)a[A_SLAB_OFF];
    uint64_t* out_bytes = (uint64_t*)a[A_OUT_BYTES]; int32_t* enc_err = (int32_t*)a[A_ENC_ERR];
    uint32_t* crc_new = (uint32_t*)a[A_CRC_NEW]; uint64_t* seg_dst = (uint64_t*)a[A_SEG_DST];
    uint64_t* seg_src = (uint64_t*)a[A_SEG_SRC]; uint64_t* seg_len = (uint64_t*)a[A_SEG_LEN]; uint8_t* slabs = (uint8_t*)a[A_SLABS];
    const uint64_t record = dict != nullptr ? 8 : 0;
    if (avail < 32 + 8 * (uint64_t)n + record) { return 7; }
    const uint64_t bb = 1ull << block_bits;
    sqzk::launch_append_plan(frame, n, content_bytes, data_bytes, block_bits, win_bits, bitmap, wpre, sel, ctl, nullptr);
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
                                 bitmap, wpre, sel, ctl, 1, in_off, out_off, skip, stored, status, blocks_encoded, nullptr,
                                 block_bits);
    if (touched != 0) {
        sqzk::launch_entropy_decode(frame, in_off, out_off, tokens, counts, err, nullptr, 2, 0, 1, nullptr, skip, dict_bytes);
        sqzk::launch_lz_expand(tokens, counts, staging, out_off, 2, nullptr, skip, dict, dict_bytes);
        sqzk::launch_range_copy(frame, in_off, staging, out_off, out_off, stored, 2, false, bb, nullptr);
        sqzk::launch_crc32_blocks(staging, out_off, 2, crc, bb, nullptr);
    }
    sqzk::launch_append_verdict(frame, n, ctl, err, crc, block_bits, content_bytes, data_bytes, m, slab_bytes, status,
                                blocks_encoded, copy, enc_in_off, slab_off, nullptr);
    if (m > 0) {
        sqzk::launch_range_copy(data, copy, staging, copy + 1, copy + 2, (const uint32_t*)(copy + 4), 1, false, data_bytes,
                                nullptr);
        sqzk::launch_crc32_blocks(staging, enc_in_off, m, crc_new, bb, nullptr);
    }
    sqzk::launch_frame_append_index(frame, n, content_bytes, data_bytes, m, dict != nullptr, out_bytes, enc_err, crc_new,
                                    slab_bytes, new_frame, capacity, seg_dst, seg_src, seg_len, new_idx_off, frame_bytes,
                                    status, nullptr);
    const uint64_t new_idx_bytes = 8 * (uint64_t)n_new + record;
    sqzk::launch_crc32_blocks(new_frame, new_idx_off, 1, &new_idx_crc, new_idx_bytes, nullptr);
    sqzk::launch_frame_seal(new_frame, &new_idx_crc, n_new, status, nullptr, (uint32_t)record);
    const uint64_t payload_off = (32 + new_idx_bytes + 15) & ~(uint64_t)15;
    sqzk::launch_frame_splice_segments(frame, slabs, staging, new_frame, seg_dst, seg_src, seg_len, m + 1,
                                       capacity > payload_off ? capacity - payload_off : 0, nullptr);
    return 0;
}
}
