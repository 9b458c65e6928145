/* tests/emu/emu_frame.cpp -- TEST INFRASTRUCTURE ONLY: the frame kernels of sqz_amd/csrc/frame.hip (checksums,
 * index construction, index validation), compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h). */
#include "hip/hip_runtime.h"

/* lanes run one after the other between two rendezvous: a plain read-modify-write is atomic here */
template <class T> inline T atomicXor(T* p, T v) { const T o = *p; *p = (T)(o ^ v); return o; }

#include "../../sqz_amd/csrc/frame.hip"

extern "C" {
int emu_crc32_blocks(const uint8_t* in, const uint64_t* off, uint32_t n, uint32_t* crc, uint64_t size_hint) {
    sqzk::launch_crc32_blocks(in, off, n, crc, size_hint, nullptr);
    return 0;
}
/* the encode side's three steps behind the emit kernel: index, checksum of the index, seal.
 * work: 2 uint64 (idx_off) + 1 uint32 (idx_crc) */
int emu_frame_index(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n,
                    uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint8_t* frame,
                    uint64_t capacity, uint64_t* copy_bytes, uint64_t* dense_off, uint64_t* frame_bytes,
                    int32_t* status) {
    uint64_t idx_off[2] = {0, 0};
    uint32_t idx_crc = 0;
    sqzk::launch_frame_index(out_bytes, err, crc, n, content_bytes, win_bits, block_bits, frame, capacity,
                             copy_bytes, dense_off, idx_off, frame_bytes, status, nullptr);
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    sqzk::launch_frame_seal(frame, &idx_crc, n, status, nullptr);
    return 0;
}
/* the decode side's first two steps: checksum of the index, open */
int emu_frame_open(const uint8_t* frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                   uint32_t n_sel, uint64_t* in_off, uint64_t* out_off, int32_t* status) {
    const uint64_t idx_off[2] = {32, 32 + 8 * (uint64_t)n};
    uint32_t idx_crc = 0;
    if (avail < idx_off[1]) { return 7; }
    sqzk::launch_crc32_blocks(frame, idx_off, 1, &idx_crc, 0, nullptr);
    sqzk::launch_frame_open(frame, avail, n, content_bytes, first, n_sel, &idx_crc, in_off, out_off, status, nullptr);
    return 0;
}
int emu_frame_verify(const uint8_t* frame, uint32_t first, uint32_t n_sel, const uint32_t* crc, const int32_t* status,
                     int32_t* err) {
    sqzk::launch_frame_verify(frame, first, n_sel, crc, status, err, nullptr);
    return 0;
}
}
