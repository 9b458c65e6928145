// tests/harness/sort_bases_check.cpp -- sqz_amd/csrc/sort_bases.h against histograms counted from the keys.
//
// index_sort_kernel counts the digit of pass 0 per position and derives the histograms of passes 1 and 2 from that
// one (sort_bases.h).  This program does the same on the host -- pass 0 counted directly, the other two through the
// header with (tid, n_threads) = (0, 1) and again with several "threads" one after another -- and compares all three
// with histograms counted directly from the keys, for both splits (10 + 7 + 7 and 8 + 8 + 8) whatever the length:
// the header does not know which lengths the kernel gives to which split.
// Exit status 0 and a last line "ok", or 1 on the first difference or bin below zero.
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined (tests/test_sort_bases_cpu.py).
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../sqz_amd/csrc/sort_bases.h"

namespace {

constexpr int kBins = 1024;               // kSortBins of lz77_index.hip

struct Rng {                              // xorshift64*
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 2685821657736338717ull) >> 32); }
};

typedef std::vector<uint8_t> Block;

Block uniform(size_t n, Rng& r) { Block b(n); for (auto& x : b) { x = (uint8_t)r.next(); } return b; }
// 0x00 .. 0x04: bytes that differ in exactly the bits that move between the digits of 10 + 7 + 7
Block five_values(size_t n, Rng& r) { Block b(n); for (auto& x : b) { x = (uint8_t)(r.next() % 5u); } return b; }
Block constant(size_t n, uint8_t v) { return Block(n, v); }
// skewed (the smallest of four draws), all below 0xF0
Block skewed(size_t n, Rng& r) {
    Block b(n);
    for (auto& x : b) {
        uint32_t v = 0xEFu;
        for (int i = 0; i < 4; i++) { const uint32_t d = r.next() % 0xF0u; v = d < v ? d : v; }
        x = (uint8_t)v;
    }
    return b;
}
uint8_t most_frequent(const Block& b) {
    size_t cnt[256] = {0};
    for (uint8_t x : b) { cnt[x]++; }
    int best = 0;
    for (int v = 1; v < 256; v++) { if (cnt[v] > cnt[best]) { best = v; } }
    return (uint8_t)best;
}
// the four end-byte blocks over a skewed body: head and tail bytes that occur nowhere else (every correction moves a
// bin the marginal leaves wrong by one), the head only, the tail only, all four ends the body's most frequent byte
Block end_bytes(size_t n, Rng& r, int which) {
    Block b = skewed(n, r);
    if (which == 3) {
        const uint8_t m = most_frequent(b);
        b[0] = b[1] = b[n - 2] = b[n - 1] = m;
        return b;
    }
    if (which == 0 || which == 2) { b[n - 2] = 0xFE; b[n - 1] = 0xFF; }     // (n == 4, 5: the head overwrites part of it)
    if (which == 0 || which == 1) { b[0] = 0xFB; b[1] = 0xFD; }
    return b;
}

bool check(const Block& b, bool small, const char* what) {
    const size_t n = b.size();
    const uint32_t w0 = small ? 10 : 8, w1 = small ? 7 : 8;
    const uint32_t m0 = (1u << w0) - 1u, m1 = (1u << w1) - 1u;
    std::vector<uint32_t> want[3], g0(kBins, 0u);
    for (auto& w : want) { w.assign(kBins, 0u); }
    for (size_t k = 0; k + 3 <= n; k++) {
        const uint32_t key = ((uint32_t)b[k] << 16) | ((uint32_t)b[k + 1] << 8) | (uint32_t)b[k + 2];
        want[0][key & m0]++;
        want[1][(key >> w0) & m1]++;
        want[2][key >> (w0 + w1)]++;
        g0[key & m0]++;                                    // the kernel's sweep
    }
    const sqzk::SortEnds ends = {b[0], b[1], b[n - 2], b[n - 1]};
    for (int n_threads : {1, 7, 1024}) {
        std::vector<uint32_t> g1(kBins, 0xDEADBEEFu), g2(kBins, 0xDEADBEEFu);
        for (int tid = 0; tid < n_threads; tid++) {
            sqzk::sort_bases_derive(g0.data(), g1.data(), g2.data(), small, ends, tid, n_threads);
        }
        const int bins = 1 << w1;                          // the bins the later passes use
        const std::vector<uint32_t>* got[3] = {&g0, &g1, &g2};
        for (int p = 0; p < 3; p++) {
            for (int d = 0; d < (p == 0 ? 1 << w0 : bins); d++) {
                const uint32_t v = (*got[p])[d];
                if ((int32_t)v < 0 || v != want[p][d]) {
                    printf("FAIL %s n=%zu %s threads=%d pass %d bin %d: derived %d, counted %u\n", what, n,
                           small ? "10+7+7" : "8+8+8", n_threads, p, d, (int32_t)v, want[p][d]);
                    return false;
                }
            }
        }
        for (int d = bins; d < kBins; d++) {               // nothing written outside the pass's bins
            if (g1[d] != 0xDEADBEEFu || g2[d] != 0xDEADBEEFu) {
                printf("FAIL %s n=%zu %s threads=%d: bin %d written\n", what, n, small ? "10+7+7" : "8+8+8", n_threads, d);
                return false;
            }
        }
    }
    return true;
}

}  // namespace

int main() {
    Rng r = {0x9E3779B97F4A7C15ull};
    std::vector<size_t> lengths;
    for (size_t n = 4; n <= 40; n++) { lengths.push_back(n); }
    for (size_t n : {4097u, 4098u, 4099u, 50001u}) { lengths.push_back(n); }
    size_t cases = 0;
    for (size_t n : lengths) {
        for (int small = 0; small < 2; small++) {
            bool ok = check(uniform(n, r), small, "uniform") && check(five_values(n, r), small, "0x00..0x04") &&
                      check(constant(n, 0xFF), small, "all 0xFF");
            static const char* const names[4] = {"ends: head and tail", "ends: head", "ends: tail", "ends: most frequent"};
            for (int which = 0; ok && which < 4; which++) { ok = check(end_bytes(n, r, which), small, names[which]); }
            if (!ok) { return 1; }
            cases += 7;
        }
    }
    printf("%zu blocks, both splits\nok\n", cases);
    return 0;
}
