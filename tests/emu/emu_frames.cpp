/* tests/emu/emu_frames.cpp -- TEST INFRASTRUCTURE ONLY: the kernels of a batch of frames (sqz_amd/csrc/frame.hip,
 * "batches of frames") -- the two scans, the plan, the index with its seal, the open and the verify for k frames --
 * each by itself, compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h).  Every array is the caller's own
 * allocation, so that each can have its guard. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"

extern "C" {
int emu_frames_encode_scan(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits, uint32_t flags,
                           uint64_t* in_at, uint64_t* frame_at, uint32_t* base) {
    sqzk::launch_frames_encode_scan(content_bytes, k, block_bits, flags, in_at, frame_at, base, nullptr);
    return 0;
}
int emu_frames_plan(const uint64_t* content_bytes, const uint64_t* in_at, const uint32_t* base, uint32_t k,
                    uint32_t block_bits, uint64_t slab_bytes, uint64_t* in_off, uint64_t* slab_off) {
    sqzk::launch_frames_plan(content_bytes, in_at, base, k, block_bits, slab_bytes, in_off, slab_off, nullptr);
    return 0;
}
int emu_frames_index(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, const uint64_t* content_bytes,
                     const uint64_t* frame_at, const uint32_t* base, uint32_t k, uint32_t win_bits, uint32_t block_bits,
                     uint32_t flags, uint8_t* frames, uint64_t* copy_bytes, uint64_t* dense_rel, uint64_t* dense_off,
                     uint32_t* stored, uint64_t* frame_bytes, int32_t* status) {
    sqzk::launch_frames_index(out_bytes, err, crc, content_bytes, frame_at, base, k, win_bits, block_bits, flags, frames,
                              copy_bytes, dense_rel, dense_off, stored, frame_bytes, status, nullptr);
    return 0;
}
int emu_frames_decode_scan(const sqz_frames_item* items, uint32_t k, uint32_t* base) {
    sqzk::launch_frames_decode_scan(items, k, base, nullptr);
    return 0;
}
int emu_frames_open(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                    uint64_t out_base, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                    int32_t* status) {
    sqzk::launch_frames_open(frames, items, base, k, out_base, in_off, out_off, skip, stored, status, nullptr);
    return 0;
}
int emu_frames_verify(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                      const uint32_t* crc, const int32_t* status, const int32_t* err, int32_t* err_out) {
    sqzk::launch_frames_verify(frames, items, base, k, crc, status, err, err_out, nullptr);
    return 0;
}
}
