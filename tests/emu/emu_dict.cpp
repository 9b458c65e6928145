/* tests/emu/emu_dict.cpp -- TEST INFRASTRUCTURE ONLY: the shared-dictionary kernels compiled for the CPU wave
 * emulator (tests/emu/hip/hip_runtime.h): dict_match_kernel behind index_match_kernel, both parses over the merged
 * table (sqz_amd/csrc/lz77_index.hip), and the decoder with a history -- the entropy kernels' `history` argument and
 * the dictionary instantiation of lz_expand_kernel (sqz_amd/csrc/decode.hip).  The caller brings the sorted
 * positions of the blocks and of the dictionary, as for emu_index.cpp. */
#include <hip/hip_runtime.h>

/* the sort's __shfl (the value of lane `src`), through the emulator's ds_bpermute */
inline int __shfl(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }

#define SQZ_DICT_THREADS 512          /* the emulator runs workgroups of up to 8 waves */
#include "../../sqz_amd/csrc/lz77_index.hip"
#include "../../sqz_amd/csrc/decode.hip"

extern "C" {
int emu_index_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, uint32_t window,
                    const uint32_t* sorted, uint32_t* match, uint32_t groups, uint64_t slots) {
    sqzk::launch_index_match(in, in_off, n_blocks, window, sorted, match, groups, slots, nullptr);
    return 0;
}
int emu_dict_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, uint32_t window,
                   const uint8_t* dict, uint32_t dict_bytes, const uint32_t* dict_sorted, uint32_t* match,
                   uint64_t slots) {
    sqzk::launch_dict_match(in, in_off, n_blocks, window, dict, dict_bytes, dict_sorted, match, slots, nullptr);
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
/* the dictionary instantiation of lz_expand_kernel alone, on the caller's token words (dict_bytes = 0: the plain one) */
int emu_expand_dict(const uint32_t* tokens, const uint32_t* tok_count, uint8_t* out, const uint64_t* out_off,
                    uint32_t n_blocks, const uint8_t* dict, uint32_t dict_bytes) {
    sqzk::launch_lz_expand(tokens, tok_count, out, out_off, n_blocks, nullptr, nullptr, dict, dict_bytes);
    return 0;
}
/* entropy decode with `history` = dict_bytes, then the expansion */
int emu_decode_dict(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint8_t* out, const uint64_t* out_off,
                    uint32_t* tokens, uint32_t* tok_count, int32_t* err, int waves, const uint8_t* dict,
                    uint32_t dict_bytes) {
    sqzk::launch_entropy_decode(in, in_off, out_off, tokens, tok_count, err, nullptr, n, 0, waves, nullptr, nullptr,
                                dict_bytes);
    sqzk::launch_lz_expand(tokens, tok_count, out, out_off, n, nullptr, nullptr, dict, dict_bytes);
    return 0;
}
int emu_dict_threads(void) { return sqzk::kDictThreads; }
}
