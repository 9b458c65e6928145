/* tests/emu/emu_index.cpp -- TEST INFRASTRUCTURE ONLY: index_match_kernel and index_parse_kernel of
 * sqz_amd/csrc/lz77_index.hip, compiled for the CPU wave emulator (tests/emu/hip/hip_runtime.h).
 * index_sort_kernel is compiled but never launched here: its workgroup has 16 waves and the emulator
 * runs up to 8, so the caller brings the sorted positions. */
#include <hip/hip_runtime.h>

/* the sort's __shfl (the value of lane `src`), through the emulator's ds_bpermute */
inline int __shfl(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

#include "../../sqz_amd/csrc/lz77_index.hip"

extern "C" {
int emu_index_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, uint32_t window,
                    const uint32_t* sorted, uint32_t* match, uint32_t groups, uint64_t slots) {
    sqzk::launch_index_match(in, in_off, n_blocks, window, sorted, match, groups, slots, nullptr);
    return 0;
}
int emu_index_parse(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, const uint32_t* match,
                    uint32_t* tokens, uint32_t* tok_count, uint64_t slots) {
    sqzk::launch_index_parse(in, in_off, n_blocks, match, tokens, tok_count, slots, nullptr);
    return 0;
}
int emu_parse_tile(void) { return sqzk::kTile; }
}
