// tests/harness/sort_rank_check.cpp -- sqz_amd/csrc/sort_rank.h against a lane-by-lane count of equal digits.
//
// index_sort_kernel ranks a row of 64 elements by a peer mask per lane: the lanes that hold an element with the same
// digit (sort_rank.h).  The kernel gives sort_rank_peers the wave's ballot; this program gives it a ballot computed
// from all 64 lanes' digits, runs it for every lane, and compares mask, rank (peers below the lane) and count with
// what a loop over the lanes finds.  On the host the bit step is the plain expression acc | (m ^ mine), the one the
// kernel's three-input operation stands for; its eight input combinations are checked bit by bit first.
// Exit status 0 and a last line "ok", or 1 on the first difference.
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined (tests/test_sort_rank_cpu.py).
#include <stdint.h>
#include <stdio.h>
#include <initializer_list>

#include "../../sqz_amd/csrc/sort_rank.h"

namespace {

constexpr int kLanes = 64;

struct Rng {                              // xorshift64*
    uint64_t s;
    uint32_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 2685821657736338717ull) >> 32); }
    uint64_t next64() { const uint64_t h = next(); return (h << 32) | next(); }
};

// the wave's votes in the order sort_rank_peers asks for them: the lanes with an element, then key bit 0, 1, ...
struct Ballot {
    const uint32_t* digit;
    uint64_t valid;
    int call;
    uint64_t operator()(bool) {
        const int bit = call++ - 1;
        if (bit < 0) { return valid; }
        uint64_t m = 0;
        for (int l = 0; l < kLanes; l++) {
            if (sqzk::sort_rank_set(sqzk::sort_rank_mine(digit[l], bit))) { m |= 1ull << l; }
        }
        return m;
    }
};

bool check_step() {
    // bit i of a, b, c: the eight combinations of (acc, m, mine) in i's three bits
    // (on the host sort_rank_step IS the plain form, so `same` only shows that the dispatch compiles; what counts here is
    // that the plain form's truth table is 0xF6, the table the kernel gives v_bitop3_b32.  The instruction itself runs
    // only on the GPU: tests/test_index_sort_rank_gpu.py)
    const uint32_t a = 0xF0u, b = 0xCCu, c = 0xAAu;
    const uint32_t got = sqzk::sort_rank_step_plain(a, b, c), same = sqzk::sort_rank_step(a, b, c);
    for (int i = 0; i < 8; i++) {
        const bool acc = (i >> 2) & 1, m = (i >> 1) & 1, mine = i & 1;
        const bool want = acc || (m != mine);              // known to differ, or this bit differs
        if ((((got >> i) & 1u) != 0u) != want || (((same >> i) & 1u) != 0u) != want) {
            printf("FAIL step: acc %d m %d mine %d: %u, want %d\n", acc, m, mine, (got >> i) & 1u, want);
            return false;
        }
    }
    if ((got & 0xFFu) != 0xF6u) { printf("FAIL step: truth table %#x, the kernel's operation has 0xf6\n", got & 0xFFu); return false; }
    for (int bit = 0; bit < 10; bit++) {                    // the spread bit and what the ballot asks of it
        for (uint32_t d : {0u, 1u << bit, 0x3FFu, 0x3FFu & ~(1u << bit)}) {
            const bool set = (d >> bit) & 1u;
            if (sqzk::sort_rank_mine(d, bit) != (set ? 0xFFFFFFFFu : 0u) || sqzk::sort_rank_set(sqzk::sort_rank_mine(d, bit)) != set) {
                printf("FAIL mine: digit %#x bit %d\n", d, bit);
                return false;
            }
        }
    }
    return true;
}

bool check_row(const uint32_t* digit, uint64_t valid, int bits, const char* what) {
    for (int l = 0; l < kLanes; l++) {
        Ballot ballot = {digit, valid, 0};
        const bool v = (valid >> l) & 1u;
        const uint64_t got = sqzk::sort_rank_peers(digit[l], v, bits, ballot);
        if (ballot.call != bits + 1) { printf("FAIL %s: %d ballots for %d bits\n", what, ballot.call, bits); return false; }
        uint64_t want = 0;
        int below = 0, count = 0;
        for (int o = 0; o < kLanes; o++) {
            if (((valid >> o) & 1u) && digit[o] == digit[l]) { want |= 1ull << o; count++; below += o < l ? 1 : 0; }
        }
        if (!v) {                                           // nobody's peer, its own included; the kernel does not use the rest
            if ((got >> l) & 1u) { printf("FAIL %s bits=%d lane %d: a lane without an element is its own peer\n", what, bits, l); return false; }
            continue;
        }
        const int got_below = __builtin_popcountll(got & ((1ull << l) - 1ull)), got_count = __builtin_popcountll(got);
        if (got != want || got_below != below || got_count != count) {
            printf("FAIL %s bits=%d lane %d digit %#x: peers %016llx (rank %d of %d), counted %016llx (rank %d of %d)\n", what, bits,
                   l, digit[l], (unsigned long long)got, got_below, got_count, (unsigned long long)want, below, count);
            return false;
        }
    }
    return true;
}

}  // namespace

int main() {
    if (!check_step()) { return 1; }
    Rng r = {0x9E3779B97F4A7C15ull};
    size_t rows = 0;
    for (int bits : {7, 8, 10}) {
        const uint32_t top = (1u << bits) - 1u;
        uint32_t digit[kLanes];
        // one digit everywhere (the first, an odd one, the last), every lane valid / the even lanes / one lane / none
        for (uint32_t d : {0u, 1u, top}) {
            for (int l = 0; l < kLanes; l++) { digit[l] = d; }
            for (uint64_t valid : {~0ull, 0x5555555555555555ull, 1ull << 63, 1ull, 0ull}) {
                if (!check_row(digit, valid, bits, "one digit")) { return 1; }
                rows++;
            }
        }
        // every lane its own digit; digits that differ in one bit only
        for (int l = 0; l < kLanes; l++) { digit[l] = (uint32_t)l ^ top; }
        if (!check_row(digit, ~0ull, bits, "all different")) { return 1; }
        for (int l = 0; l < kLanes; l++) { digit[l] = 1u << (l % bits); }
        if (!check_row(digit, ~0ull, bits, "one bit each")) { return 1; }
        rows += 2;
        // random digits -- of the whole range, of five neighbouring values, of the first and the last -- and random valid
        // masks: all lanes, a ragged end (the first n lanes, as the kernel has them), any lanes
        for (int round = 0; round < 400; round++) {
            const int kind = round % 3;
            for (int l = 0; l < kLanes; l++) {
                const uint32_t x = r.next();
                digit[l] = kind == 0 ? x & top : kind == 1 ? x % 5u : (x & 1u) ? top : 0u;
            }
            const uint32_t n = r.next() % (kLanes + 1);
            const uint64_t ragged = n == kLanes ? ~0ull : (1ull << n) - 1ull;
            const uint64_t masks[3] = {~0ull, ragged, r.next64()};
            for (uint64_t valid : masks) {
                // the kernel gives a lane without an element digit 0
                uint32_t d[kLanes];
                for (int l = 0; l < kLanes; l++) { d[l] = ((valid >> l) & 1u) ? digit[l] : 0u; }
                if (!check_row(d, valid, bits, "random") || !check_row(digit, valid, bits, "random, digits in unused lanes")) { return 1; }
                rows += 2;
            }
        }
    }
    printf("%zu rows of 64 lanes\nok\n", rows);
    return 0;
}
