/* tests/emu/emu_frames_v4.cpp -- TEST INFRASTRUCTURE ONLY: a batch of frames with byte-shuffled (version 4) ones in it
 * -- the shuffle kernel for ranges of mixed element size (sqz_amd/csrc/shuffle.hip) and the version-4 flavours of the
 * batch's scan, plan, index and open kernels (sqz_amd/csrc/frame.hip) -- each by itself, compiled for the CPU wave
 * emulator (tests/emu/hip/hip_runtime.h).  Every array is the caller's own allocation, so that each can have its
 * guard. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/shuffle.hip"

extern "C" {
/* the launchers as the library calls them: hint = 0 (size unknown: the most workgroups a range) or the largest range */
int emu_shuffle_ranges(const uint8_t* src, const uint64_t* off, const uint32_t* elem, uint32_t n, int inverse,
                       uint8_t* dst, const uint32_t* skip, uint64_t hint) {
    sqzk::launch_shuffle_ranges(src, off, elem, n, inverse != 0, dst, skip, hint, nullptr);
    return 0;
}
int emu_shuffle_blocks(const uint8_t* src, const uint64_t* off, uint32_t n, uint32_t elem_bytes, int inverse,
                       uint8_t* dst, const uint32_t* skip, uint64_t hint) {
    sqzk::launch_shuffle_blocks(src, off, n, elem_bytes, inverse != 0, dst, skip, hint, nullptr);
    return 0;
}
int emu_frames_encode_scan_v4(const uint64_t* content_bytes, const uint32_t* elem, uint32_t k, uint32_t block_bits,
                              uint32_t flags, uint64_t* in_at, uint64_t* frame_at, uint32_t* base) {
    sqzk::launch_frames_encode_scan_v4(content_bytes, elem, k, block_bits, flags, in_at, frame_at, base, nullptr);
    return 0;
}
int emu_frames_plan_v4(const uint64_t* content_bytes, const uint32_t* elem, const uint64_t* in_at, const uint32_t* base,
                       uint32_t k, uint32_t block_bits, uint64_t slab_bytes, uint64_t* in_off, uint64_t* slab_off,
                       uint32_t* blk_elem) {
    sqzk::launch_frames_plan_v4(content_bytes, elem, in_at, base, k, block_bits, slab_bytes, in_off, slab_off, blk_elem,
                                nullptr);
    return 0;
}
int emu_frames_index_v4(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc,
                        const uint64_t* content_bytes, const uint32_t* elem, const uint64_t* frame_at,
                        const uint32_t* base, uint32_t k, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                        uint8_t* frames, uint64_t* copy_bytes, uint64_t* dense_rel, uint64_t* dense_off, uint32_t* stored,
                        uint64_t* frame_bytes, int32_t* status) {
    sqzk::launch_frames_index_v4(out_bytes, err, crc, content_bytes, elem, frame_at, base, k, win_bits, block_bits, flags,
                                 frames, copy_bytes, dense_rel, dense_off, stored, frame_bytes, status, nullptr);
    return 0;
}
int emu_frames_decode_scan(const sqz_frames_item* items, uint32_t k, uint32_t* base) {
    sqzk::launch_frames_decode_scan(items, k, base, nullptr);
    return 0;
}
int emu_frames_open_v4(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                       uint64_t out_base, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                       uint32_t* ent_elem, int32_t* status) {
    sqzk::launch_frames_open_v4(frames, items, base, k, out_base, in_off, out_off, skip, stored, ent_elem, status,
                                nullptr);
    return 0;
}
}
