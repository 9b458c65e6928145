/* tests/emu/emu_frame_v4.cpp -- TEST INFRASTRUCTURE ONLY: SQZF version 4 -- the byte-shuffle kernel
 * (sqz_amd/csrc/shuffle.hip) and the version-4 kernels of the index and open code (sqz_amd/csrc/frame.hip) --
 * compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h) and chained as sqz_amd/csrc/abi.hip chains them. */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"
#include "../../sqz_amd/csrc/shuffle.hip"

extern "C" {
/* the launcher as the library calls it: hint = 0 (size unknown: the most workgroups a range) or the largest range */
int emu_shuffle_blocks(const uint8_t* src, const uint64_t* off, uint32_t n, uint32_t elem_bytes, int inverse,
                       uint8_t* dst, const uint32_t* skip, uint64_t hint) {
    sqzk::launch_shuffle_blocks(src, off, n, elem_bytes, inverse != 0, dst, skip, hint, nullptr);
    return 0;
}
/* the encode side's steps behind the emit kernel: index, checksum of index and record, seal */
int emu_frame_index_v4(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n,
                       uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                       uint32_t elem_bytes, uint8_t* frame, uint64_t capacity, uint64_t* copy_bytes,
                       uint64_t* dense_off, uint32_t* stored, uint64_t* frame_bytes, int32_t* status) {
    uint64_t idx_off[2] = {0, 0};
    uint32_t idx_crc = 0;
    sqzk::launch_frame_index_v4(out_bytes, err, crc, n, content_bytes, win_bits, block_bits, flags, elem_bytes, frame,
                                capacity, copy_bytes, dense_off, stored, idx_off, frame_bytes, status, nullptr);
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 8 * (uint64_t)n + 8, nullptr);
    sqzk::launch_frame_seal(frame, &idx_crc, n, status, nullptr, 8);
    return 0;
}
/* the decode side's first steps: checksum of index and record, open */
int emu_frame_open_v4(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                      uint32_t n_sel, uint32_t elem_bytes, uint64_t* in_off, uint64_t* out_off, uint32_t* stored,
                      int32_t* status, uint32_t want_bits) {
    uint64_t idx_off[2] = {77, 77}, spare[2] = {0, 0};
    uint32_t idx_crc = 0;
    if (avail < 32 + 8 * (uint64_t)n + 8) { return 7; }
    sqzk::launch_frame_plan(1, 8 * (uint64_t)n + 8, 8 * (uint64_t)n + 8, 0, idx_off, spare, nullptr);
    sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, &idx_crc, 8 * (uint64_t)n + 8, nullptr);
    sqzk::launch_frame_open_v4(frame, avail, n, content_bytes, first, n_sel, &idx_crc, elem_bytes, in_off, out_off,
                               stored, status, nullptr, want_bits);
    return 0;
}
/* the launchers there were, on whatever frame they are given (every one must refuse a version-4 frame) */
int emu_frame_open_old(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                       uint32_t n_sel, uint64_t* in_off, uint64_t* out_off, uint32_t* stored, int32_t* status) {
    const uint64_t idx_off[2] = {32, 32 + 8 * (uint64_t)n};
    uint32_t idx_crc = 0;
    if (avail < idx_off[1]) { return 7; }
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    sqzk::launch_frame_open_v2(frame, avail, n, content_bytes, first, n_sel, &idx_crc, in_off, out_off, stored, status,
                               nullptr, 0);
    return 0;
}
}
