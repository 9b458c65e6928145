// sqz_amd/csrc/sort_bases.h -- index_sort_kernel: the histograms of passes 1 and 2 from the histogram of pass 0.
//
// Plain C++ (no HIP include): index_sort_kernel calls sort_bases_derive with its 1024 threads, a host program with
// (tid, n_threads) = (0, 1) -- tests/harness/sort_bases_check.cpp holds it against histograms counted from the keys.
//
// The key of position k is b[k] << 16 | b[k+1] << 8 | b[k+2], k = 0 .. n-3 (n = the block's bytes, n >= 4).
//
// 10 + 7 + 7 (blocks up to 256 KB):
//   d0 = (b[k+1] & 3) << 8 | b[k+2]     a function of the byte pair at k+1
//   d1 = (b[k] & 1) << 6 | b[k+1] >> 2  a coarser function of the byte pair at k
//   d2 = b[k] >> 1                      a function of one byte
// so the histograms of d1 and d2 are marginals of d0's (every bin the sum of eight bins of it), taken over positions one
// and two further on: d0's histogram saw the pairs at 1 .. n-2 and their second bytes 2 .. n-1, d1 wants the pairs at
// 0 .. n-3 and d2 the bytes 0 .. n-3.  The block's first two and last two bytes make up the difference.
//
// 8 + 8 + 8 (longer blocks): all three are the byte histogram, of bytes 2 .. n-1, 1 .. n-2 and 0 .. n-3.
//
// No bin goes below zero: every -1 takes out a byte or a pair that the marginal did count.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SQZ_SORT_BASES_FN __host__ __device__ inline
#else
#define SQZ_SORT_BASES_FN inline
#endif

namespace sqzk {

constexpr int kSortBasesSmallBins = 128;         // bins of passes 1 and 2, 10 + 7 + 7
constexpr int kSortBasesLargeBins = 256;         // bins of every pass, 8 + 8 + 8

struct SortEnds { uint32_t b0, b1, y0, y1; };    // the block's bytes 0, 1, n-2 and n-1

// 10 + 7 + 7: the digit of pass 1 of a position whose first two key bytes are (x, y)
SQZ_SORT_BASES_FN uint32_t sort_bases_d1(uint32_t x, uint32_t y) { return ((x & 1u) << 6) | (y >> 2); }

// 10 + 7 + 7: bin d of pass 1 -- the bins f of pass 0 with ((f >> 8) & 1) << 6 | (f & 0xFF) >> 2 == d
SQZ_SORT_BASES_FN uint32_t sort_bases_small_1(const uint32_t* g0, uint32_t d, const SortEnds& e) {
    const uint32_t f = ((d >> 6) << 8) | ((d & 63u) << 2);           // bits 9, 1 and 0 of f are free
    uint32_t sum = 0;
    for (uint32_t h = 0; h < 2; h++) {
        for (uint32_t l = 0; l < 4; l++) { sum += g0[(h << 9) | f | l]; }
    }
    sum += sort_bases_d1(e.b0, e.b1) == d ? 1u : 0u;
    sum -= sort_bases_d1(e.y0, e.y1) == d ? 1u : 0u;
    return sum;
}

// 10 + 7 + 7: bin d of pass 2 -- the bins f of pass 0 with (f & 0xFF) >> 1 == d
SQZ_SORT_BASES_FN uint32_t sort_bases_small_2(const uint32_t* g0, uint32_t d, const SortEnds& e) {
    uint32_t sum = 0;
    for (uint32_t h = 0; h < 4; h++) {                               // bits 9, 8 and 0 of f are free
        for (uint32_t l = 0; l < 2; l++) { sum += g0[(h << 8) | (d << 1) | l]; }
    }
    sum += (e.b0 >> 1 == d ? 1u : 0u) + (e.b1 >> 1 == d ? 1u : 0u);
    sum -= (e.y0 >> 1 == d ? 1u : 0u) + (e.y1 >> 1 == d ? 1u : 0u);
    return sum;
}

// 8 + 8 + 8: bin d of pass 1 and of pass 2
SQZ_SORT_BASES_FN uint32_t sort_bases_large_1(const uint32_t* g0, uint32_t d, const SortEnds& e) {
    return g0[d] + (e.b1 == d ? 1u : 0u) - (e.y1 == d ? 1u : 0u);
}
SQZ_SORT_BASES_FN uint32_t sort_bases_large_2(const uint32_t* g0, uint32_t d, const SortEnds& e) {
    return g0[d] + (e.b0 == d ? 1u : 0u) + (e.b1 == d ? 1u : 0u) - (e.y0 == d ? 1u : 0u) - (e.y1 == d ? 1u : 0u);
}

// g1 and g2 (the counts of passes 1 and 2) from g0 (the counts of pass 0, complete and no longer changing).  Thread
// `tid` of `n_threads` writes the bins it owns, end corrections included, and reads g0 only: no thread waits for
// another, and one barrier behind the call is all the caller needs.
SQZ_SORT_BASES_FN void sort_bases_derive(const uint32_t* g0, uint32_t* g1, uint32_t* g2, bool small, const SortEnds& e,
                                         int tid, int n_threads) {
    const int bins = small ? kSortBasesSmallBins : kSortBasesLargeBins;
    for (int o = tid; o < 2 * bins; o += n_threads) {
        const uint32_t d = (uint32_t)(o < bins ? o : o - bins);
        if (o < bins) { g1[d] = small ? sort_bases_small_1(g0, d, e) : sort_bases_large_1(g0, d, e); }
        else { g2[d] = small ? sort_bases_small_2(g0, d, e) : sort_bases_large_2(g0, d, e); }
    }
}

}  // namespace sqzk
