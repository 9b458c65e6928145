/* tests/emu/emu_parse_lazy.cpp -- TEST INFRASTRUCTURE ONLY: both instantiations of index_parse_kernel
 * (sqz_amd/csrc/lz77_index.hip), greedy and lazy, and index_match_kernel, compiled for the CPU wave emulator
 * (tests/emu/hip/hip_runtime.h).  The caller brings the sorted positions, as for emu_index.cpp. */
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
/* lazy: 0 = launch_index_parse (greedy), 1 = launch_index_parse_lazy */
int emu_index_parse(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, const uint32_t* match,
                    uint32_t* tokens, uint32_t* tok_count, uint64_t slots, int lazy) {
    if (lazy) {
        sqzk::launch_index_parse_lazy(in, in_off, n_blocks, match, tokens, tok_count, slots, nullptr);
    } else {
        sqzk::launch_index_parse(in, in_off, n_blocks, match, tokens, tok_count, slots, nullptr);
    }
    return 0;
}
int emu_parse_tile(void) { return sqzk::kTile; }
int emu_parse_chunk(void) { return sqzk::kChunk; }
}
