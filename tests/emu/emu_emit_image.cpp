/* tests/emu/emu_emit_image.cpp -- TEST INFRASTRUCTURE ONLY: encode stage 2 of sqz_amd/csrc/huffman_emit.hip on the
 * CPU wave emulator (tests/emu/hip/hip_runtime.h), with what tests/test_emit_image_emu.py needs beyond
 * emu_emit.cpp: the caller's output offsets (capacities cut short), the header bits of the single-stream entry,
 * and the emulator build's counters of the bit image (drains, steps of the main loop). */
#include "../../sqz_amd/csrc/huffman_emit.hip"

extern "C" {
int emu_emit_image(const uint32_t* tokens, const uint64_t* tok_off, const uint32_t* tok_count, uint32_t n,
                   uint8_t* out, const uint64_t* out_off, uint64_t* out_bytes, int32_t* err,
                   uint64_t prefix_acc, int prefix_fill, uint32_t* drains, uint32_t* steps) {
    sqzk::g_dbg_drains = 0;
    sqzk::g_dbg_steps = 0;
    sqzk::launch_huffman_emit(tokens, tok_off, tok_count, out, out_off, out_bytes, err, n, prefix_acc, prefix_fill,
                              nullptr, nullptr);
    if (drains != nullptr) { *drains = sqzk::g_dbg_drains; }
    if (steps != nullptr) { *steps = sqzk::g_dbg_steps; }
    return 0;
}
}
