// sqz_amd/csrc/sort_rank.h -- index_sort_kernel: which lanes of a wave hold the same digit (the peer mask of a row).
//
// No HIP include: index_sort_kernel calls sort_rank_peers with the wave's ballot, a host program with a ballot it
// computes itself from all 64 lanes' digits -- tests/harness/sort_rank_check.cpp holds the result against a lane-by-lane
// count of equal digits.
//
// The mask is built from the other side: `acc` collects the lanes that DIFFER from this one.  It starts as the lanes
// without an element, every key bit adds the lanes whose bit is not mine -- the ballot of the bit, m, xored with my
// own bit spread over a dword (all ones or zero): m where my bit is clear, ~m where it is set -- and what is left
// at the end are the peers.  Per bit and 32-bit half that is one three-input operation, acc | (m ^ mine), which
// gfx950 has as v_bitop3_b32 (truth table 0xF6 for the inputs a = 0xF0, b = 0xCC, c = 0xAA); everywhere else it is
// the plain expression.  The ballot tests the spread bit's sign, so the compare reads what the v_bfe_i32 left and
// needs no shift of its own: four vector instructions per bit (bfe, compare, two bitop3).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SQZ_SORT_RANK_FN __host__ __device__ inline
#else
#define SQZ_SORT_RANK_FN inline
#endif
#if defined(__clang__)
#define SQZ_SORT_RANK_UNROLL _Pragma("unroll")
#else
#define SQZ_SORT_RANK_UNROLL
#endif

namespace sqzk {

// bit `bit` of the digit over a whole dword: all ones when it is set
SQZ_SORT_RANK_FN uint32_t sort_rank_mine(uint32_t digit, int bit) {
    return (uint32_t)((int32_t)(digit << (31 - bit)) >> 31);
}

// what the ballot of a bit asks of a lane
SQZ_SORT_RANK_FN bool sort_rank_set(uint32_t mine) { return (int32_t)mine < 0; }

// one bit, one half of the mask: the lanes known to differ (acc) and those whose bit (m) is not mine
SQZ_SORT_RANK_FN uint32_t sort_rank_step_plain(uint32_t acc, uint32_t m, uint32_t mine) { return acc | (m ^ mine); }

SQZ_SORT_RANK_FN uint32_t sort_rank_step(uint32_t acc, uint32_t m, uint32_t mine) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__) && !defined(SQZ_WAVE_EMU)
    return __builtin_amdgcn_bitop3_b32(acc, m, mine, 0xF6);
#else
    return sort_rank_step_plain(acc, m, mine);
#endif
}

// lanes of this wave that are valid and hold the same digit (of `bits` bits), as a 64-bit mask.  `ballot(p)` is the
// wave's vote: bit l set when lane l passed true.  A lane without an element is nobody's peer (its own result is not
// used).  The function is marked for host and device so that the host check can call it; the kernel passes a lambda
// around __ballot, which exists on the device only -- a template is compiled for the side that instantiates it, so
// the host never sees that lambda's body.
template <class Ballot>
SQZ_SORT_RANK_FN uint64_t sort_rank_peers(uint32_t digit, bool valid, int bits, Ballot&& ballot) {
    const uint64_t none = ~ballot(valid);
    uint32_t lo = (uint32_t)none, hi = (uint32_t)(none >> 32);
    SQZ_SORT_RANK_UNROLL
    for (int bit = 0; bit < 10; bit++) {
        if (bit < bits) {
            const uint32_t mine = sort_rank_mine(digit, bit);
            const uint64_t m = ballot(sort_rank_set(mine));
            lo = sort_rank_step(lo, (uint32_t)m, mine);
            hi = sort_rank_step(hi, (uint32_t)(m >> 32), mine);
        }
    }
    return ~(((uint64_t)hi << 32) | lo);
}

}  // namespace sqzk
