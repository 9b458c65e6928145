// sqz_amd/csrc/lz77_index.hip -- encode stage 1, indexed form (gfx950).
//
// Same result as the brute-force scan of lz77_scan.hip (and therefore as the
// reference, attic/map_experiment/squeeze.h:338-358,377-394), found without
// visiting every distance: a candidate can only matter if it shares the first
// 3 bytes with the string at i (squeeze_deflate_len_min = 3, squeeze.h:13), so
// it is enough to visit, nearest first, the earlier positions with the same
// 3-byte prefix.  This is SURVEY.md section 8f-3 ("faster exact match
// finders ... every in-window candidate sharing the 3-byte prefix visited
// nearest-first with strict >"), validated like bst.c:254-308 validates its
// finder: token-for-token equality with the brute-force scan (tests).
//
// Three kernels:
//   index_sort_kernel   one 1024-thread workgroup per stream: stable LSD radix
//                       sort (3 passes: 10 + 7 + 7 key bits for blocks of up to 256 KB,
//                       8 + 8 + 8 for longer ones) of the positions 0..n-3 by their
//                       3-byte prefix; the three histograms come from one sweep over
//                       the bytes, every pass orders 4096-element tiles in LDS so that
//                       a digit's elements leave as contiguous runs.  Equal prefixes
//                       end up adjacent, positions ascending inside a run.
//   index_match_kernel  one thread per position (all positions, not only token
//                       starts -- there is no serial dependence here): walk the
//                       run backwards = nearest first, stop at distance
//                       min(i, window-1), keep the first strictly longer match,
//                       stop at len == min(bytes-i, 257).  -> match[i].  A wave whose
//                       64 ranks lie inside one run walks the candidates once for
//                       all its lanes; a stream's workgroups share one XCD.  A wave's
//                       pages cost a fixed two loads and one store each, the loads issued
//                       one and two pages ahead, and nothing waits for the scattered store
//                       of the page before.
//   index_parse_kernel  one wavefront per stream: the greedy step
//                       (squeeze.h:377-394) over match[] -> the token words of
//                       stage 1 (same format as lz77_scan.hip), found by per-chunk
//                       walks that merge with the real path instead of one serial walk.
#include "sqz_device.h"
#include "sqz_kernels.h"
#include "sort_bases.h"
#include "sort_rank.h"

namespace sqzk {

constexpr int kSharedGiveUp = 8;         // index_match: lanes gone their own way before a wave stops sharing its walk
constexpr int kXcds = 8;                 // MI355X: 8 XCDs, workgroups dispatched round-robin over them
constexpr int kSortThreads = 1024;
constexpr int kSortWaves = kSortThreads / kWave;

constexpr int kSortTile = 4 * kSortThreads;      // elements per workgroup tile (4 rows of 64 per wave)

// The three digit histograms do not depend on the order of the elements (a position's key
// bytes are fixed), so one sweep over the stream's BYTES gives all three (it counts the digit of
// pass 0; the other two histograms are sums of bins of that one: sort_bases.h); each pass is then a
// single sweep over the elements.  The scatter does not write elements where they fall: every
// 4096-element tile is first ordered by digit in LDS (stable: wave order, then row and lane order
// inside a wave), then copied out, so a digit's elements of one tile leave as one contiguous run.
// Writing each element straight to its bucket kept ~256 half-filled lines open per wave -- 16 MB
// of open lines per XCD against 4 MB of L2 -- and they left as partial-line writes: 53 GB written
// for 12 GB of elements.
//
// Which key bits a pass sorts by is free: all that is needed is that equal 24-bit keys end up
// adjacent with positions ascending (a stable LSD sort over ANY split of the 24 bits).  Blocks of
// up to 256 KB (positions < 2^18) use 10 + 7 + 7 bits: pass 0 reads the positions in order, so the
// whole key is at hand, and the 14 bits it does not sort by travel in the element's top bits -- the
// later passes never gather a byte at random (those gathers were half of the kernel's 28.8 GB of
// fetches: 64 streams of 256 KB per XCD against 4 MB of L2).  Longer blocks use 8 + 8 + 8: pass 1
// gathers bytes p and p+1 and carries byte 0 (blocks up to 16 MB), pass 2 of longer ones gathers.
//
// A tile costs four workgroup barriers, and every thread works between any two of them: the waves rank
// their own 256 elements (per-wave counters), ONE workgroup-wide exclusive scan over the bins x 16
// counters in digit-major order turns every (wave, digit) counter into the tile slot of that wave's first
// element of the digit (a thread owns 16, 4 or 2 counters of one digit), the elements go to their slots,
// and the slots leave in order.  The barriers wait for LDS only: the tile's stores drain while the next
// tile is ranked, and the next tile's loads are issued before this tile's ranking and consumed after its
// copy-out, so no HBM round trip stands behind a barrier.  Only the pass boundary waits for the stores.
constexpr int kSortBins = 1024;                  // most digits of a pass
constexpr int kSortCntRow = kSortBins + 2;       // a wave's counters start one LDS bank after the wave's before (the scan reads a digit's 16 side by side)
struct SortLds {
    uint32_t elem[kSortTile];                    // the tile in digit order
    uint16_t dig[kSortTile];                     // digit per tile slot
    uint16_t cnt[kSortWaves][kSortCntRow];       // per tile: elements of (wave, digit) so far; after the scan: tile slot of the first of them
    uint32_t gbase[3][kSortBins];                // per pass: where the next tile's run of digit d goes
    uint32_t delta[kSortBins];                   // per tile: (index in the pass's output) - (tile slot) of digit d's run
    uint32_t wtot[kSortWaves];                   // the scan's hand-over: elements counted by each wave's threads
};                                               // 72 KB: two workgroups per CU

struct __attribute__((packed)) U32u { uint32_t v; };

__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t* p) {
    return reinterpret_cast<const U32u*>(p)->v;
}

// lanes of this wave with the same digit (of `bits` bits) and valid, as a 64-bit mask (sort_rank.h).  Per bit: the
// lane's bit spread over a dword (one v_bfe_i32), one ballot of its sign, and per half of the mask one v_bitop3_b32.
__device__ __forceinline__ uint64_t peers_of(uint32_t digit, bool valid, int bits) {
    return sort_rank_peers(digit, valid, bits, [](bool p) { return (uint64_t)__ballot(p); });
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {   // popcount of mask below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// the key of position k as one number: byte k first (most significant), byte k+2 last
__device__ __forceinline__ uint32_t sort_key(const uint8_t* src, uint64_t bytes, uint32_t k) {
    return (uint64_t)k + 4 <= bytes ? (__builtin_bswap32(load_u32_unaligned(src + k)) >> 8)
                                    : (((uint32_t)src[k] << 16) | ((uint32_t)src[k + 1] << 8) | (uint32_t)src[k + 2]);
}

typedef uint32_t __attribute__((may_alias)) SortCntPair;      // two neighbouring uint16 counters, zeroed together

// Section timers of the instrumented build (tools/build_stats.sh): cycles of wave 0 of block 1 per section, each
// section including the barrier that ends it.  0 histogram sweep + bucket bases; per tile: 1 the tile's loads have
// arrived (the instrumented build waits for them there: vmcnt(0), which also waits for the tile's stores before),
// 2 rank, 3 scan (own counters), 4 scan (hand-over, slot bases), 5 place, 6 copy-out (issue only: no barrier).
struct SortSec {
#ifdef SQZ_STATS
    uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t last = 0;
#endif
};
#ifdef SQZ_STATS
#define SORT_SEC(s, k) { const uint64_t n_ = __builtin_readcyclecounter(); (s).t[k] += n_ - (s).last; (s).last = n_; }
#define SORT_SEC_LOADS(s, k) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); SORT_SEC(s, k) }
#else
#define SORT_SEC(s, k)
#define SORT_SEC_LOADS(s, k)
#endif

// One pass: the elements of `from` (pass 0: the positions in order), by the pass's digit of kBits bits, to `to`.
// kSmall: the 10 + 7 + 7 split of blocks up to 256 KB (kBits == 10 is its pass 0); else 8 + 8 + 8.
template <int kBits, bool kSmall>
__device__ __forceinline__ void sort_pass(SortLds& lds, const int pass, const uint8_t* __restrict__ src,
                                          const uint64_t bytes, const uint32_t count, const bool carry,
                                          const uint32_t* __restrict__ from, uint32_t* __restrict__ to, SortSec& sec) {
    constexpr int kDigits = 1 << kBits;
    constexpr int kTpd = kSortThreads / kDigits;       // the scan: threads per digit (1, 8 or 4) ...
    constexpr int kWpt = kSortWaves / kTpd;            // ... and waves' counters per thread (16, 2 or 4)
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool first = kSmall ? kBits == 10 : pass == 0;
    uint32_t* const gbase = lds.gbase[pass];

    // element k of the input order belongs to tile k / 4096, wave (k / 256) % 16, row (k / 64) % 4.
    // What a tile needs from memory, one dword per row: the key (pass 0) or the element.
    // Every lane loads, from a clamped address, so that the four loads are issued back to back with nothing waiting
    // on them: a row past the end reads the last element again and is not used.  Pass 0 reads the dword at k, whose
    // first three bytes are the key; the last position has no fourth byte and reads the dword one byte earlier
    // (bytes >= 4: the kernel deals with a 3-byte block by itself).
    auto fetch = [&](uint32_t tile, uint32_t (&raw)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t k = tile + (uint32_t)(wave * 256 + j * kWave + lane);
            if (first) {
                const uint32_t last = (uint32_t)(bytes - 4);
                raw[j] = load_u32_unaligned(src + (k < last ? k : last));
            } else {
                raw[j] = from[k < count ? k : count - 1u];
            }
        }
    };
    auto key_from = [&](uint32_t raw, uint32_t k) {
        const uint32_t be = __builtin_bswap32(raw);
        return (uint64_t)k + 4 <= bytes ? be >> 8 : be & 0x00FFFFFFu;
    };
    auto decode = [&](uint32_t tile, const uint32_t (&raw)[4], uint32_t (&elem)[4], uint32_t (&digit)[4], bool (&valid)[4]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t k = tile + (uint32_t)(wave * 256 + j * kWave + lane);
            valid[j] = k < count;
            const uint32_t pos = valid[j] ? (first ? k : raw[j]) : 0u;
            digit[j] = 0; elem[j] = pos;
            if (!valid[j]) { continue; }
            if (kSmall) {
                if (first) {
                    const uint32_t key = key_from(raw[j], k);
                    digit[j] = key & 0x3FFu;
                    elem[j] = pos | ((key >> 10) << 18);                 // 14 key bits above an 18-bit position
                } else if (pass == 1) {
                    digit[j] = (pos >> 18) & 0x7Fu;
                } else {
                    digit[j] = pos >> 25;
                    elem[j] = pos & 0x3FFFFu;
                }
            } else if (first) {
                digit[j] = key_from(raw[j], k) & 0xFFu;                  // byte k+2
            } else if (pass == 1) {                                      // the one random gather: bytes p and p+1
                const uint32_t w = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8);
                digit[j] = w >> 8;
                if (carry) { elem[j] = pos | ((w & 0xFFu) << 24); }
            } else {
                digit[j] = carry ? (pos >> 24) : (uint32_t)src[pos];
                if (carry) { elem[j] = pos & 0x00FFFFFFu; }
            }
        }
    };

    // A tile's dwords are loaded one tile ahead and turned into elements and digits at the END of the tile before, behind
    // that tile's stores: the wait is for the four loads in front of the stores, and no wave ever waits for a store.
    uint32_t ahead[4], elem[4], digit[4], wrank[4];
    bool valid[4];
    fetch(0u, ahead);
    decode(0u, ahead, elem, digit, valid);
    SORT_SEC_LOADS(sec, 1)
    for (uint32_t tile = 0; tile < count; tile += (uint32_t)kSortTile) {
        const uint32_t n_tile = count - tile < (uint32_t)kSortTile ? count - tile : (uint32_t)kSortTile;
        fetch(tile + (uint32_t)kSortTile, ahead);          // (past the last tile: the last element, four times)
        {   // this wave's counters: nobody else looks at them between the last barrier of a tile and the first of the next
            SortCntPair* const row = reinterpret_cast<SortCntPair*>(lds.cnt[wave]);
            for (int d = lane; d < kDigits / 2; d += kWave) { row[d] = 0u; }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {                      // rows in order: stability
            const uint64_t peers = peers_of(digit[j], valid[j], kBits);
            const uint32_t rank = lanes_below(peers);
            wrank[j] = valid[j] ? (uint32_t)lds.cnt[wave][digit[j]] + rank : 0u;
            __builtin_amdgcn_wave_barrier();               // all reads before the leaders' writes
            if (valid[j] && rank == 0) {
                lds.cnt[wave][digit[j]] = (uint16_t)(lds.cnt[wave][digit[j]] + (uint32_t)__builtin_popcountll(peers));
            }
            __builtin_amdgcn_wave_barrier();
        }
        lds_barrier();
        SORT_SEC(sec, 2)
        // exclusive scan over the counters in (digit, wave) order: thread t owns kWpt waves' counters of one digit
        const int sd = tid / kTpd;
        const int sw = (tid % kTpd) * kWpt;
        uint32_t c[kWpt], sum = 0;
#pragma unroll
        for (int i = 0; i < kWpt; i++) { c[i] = lds.cnt[sw + i][sd]; sum += c[i]; }
        const uint32_t incl = wave_scan(sum);
        if (lane == kWave - 1) { lds.wtot[wave] = incl; }
        lds_barrier();
        SORT_SEC(sec, 3)
        uint32_t at = wave_scan(lane < wave ? lds.wtot[lane] : 0u);          // the waves in front of this one
        at = (uint32_t)__builtin_amdgcn_readlane((int)at, kWave - 1) + incl - sum;
        const uint32_t run = at;                           // (of the digit's first thread: where its run starts in the tile)
#pragma unroll
        for (int i = 0; i < kWpt; i++) { lds.cnt[sw + i][sd] = (uint16_t)at; at += c[i]; }
        const uint32_t run_end = kTpd > 1 ? (uint32_t)__shfl((int)at, lane | (kTpd - 1)) : at;
        if (tid % kTpd == 0) {                             // the run's place in the output, and the next tile's
            const uint32_t g = gbase[sd];
            lds.delta[sd] = g - run;
            gbase[sd] = g + (run_end - run);
        }
        lds_barrier();
        SORT_SEC(sec, 4)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (valid[j]) {
                const uint32_t slot = (uint32_t)lds.cnt[wave][digit[j]] + wrank[j];
                if (slot < (uint32_t)kSortTile) {          // always: slots are a permutation of [0, n_tile)
                    lds.elem[slot] = elem[j];
                    lds.dig[slot] = (uint16_t)digit[j];
                }
            }
        }
        lds_barrier();
        SORT_SEC(sec, 5)
        // Runs leave contiguously.  Every lane stores, so that the four stores are issued back to back and what follows
        // can tell them from the loads in front of them: a slot past the tile's end stores the tile's last element
        // again, and the clamp never acts (slot -> index is a permutation of [0, count)): it only keeps a store inside
        // the stream's array whatever the counters hold.
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t slot = (uint32_t)(j * kSortThreads + tid);
            const uint32_t s = slot < n_tile ? slot : n_tile - 1u;
            const uint32_t dest = s + lds.delta[lds.dig[s]];
            to[dest < count ? dest : count - 1u] = lds.elem[s];
        }
        SORT_SEC(sec, 6)
        decode(tile + (uint32_t)kSortTile, ahead, elem, digit, valid);
        SORT_SEC_LOADS(sec, 1)
    }
    // the next pass reads what other waves of this workgroup wrote
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(kSortThreads)
void index_sort_kernel(const uint8_t* __restrict__ in,
                       const uint64_t* __restrict__ in_off,
                       uint32_t n_blocks,
                       uint32_t* __restrict__ buf_a,      // result lands here
                       uint32_t* __restrict__ buf_b,
                       uint64_t slots) {
    __shared__ SortLds lds;
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks || in_off[b + 1] > slots) { return; }   // beyond the caller's arrays: index_parse refuses the block
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const uint8_t* src = in + in_off[b];
    const uint64_t bytes = in_off[b + 1] - in_off[b];
    if (bytes < 3) { return; }
    const uint32_t count = (uint32_t)(bytes - 2);             // positions with a 3-byte prefix
    uint32_t* const pa = buf_a + in_off[b];
    uint32_t* const pb = buf_b + in_off[b];
    if (bytes == 3) {                                         // one position (and no dword to read its key from)
        if (tid == 0) { pa[0] = 0u; }
        return;
    }
    const bool small = bytes <= (1u << 18);                   // the unsorted key bits fit above the position
    const bool carry = bytes <= (1u << 24);                   // (8 + 8 + 8) byte 0 fits above the position
    // pass p sorts by key bits [shift[p], shift[p] + width[p])
    const int w0 = small ? 10 : 8, w1 = small ? 7 : 8, w2 = small ? 7 : 8;
    const uint32_t m0 = (1u << w0) - 1u;
    SortSec sec;
#ifdef SQZ_STATS
    sec.last = __builtin_readcyclecounter();
    const uint64_t sec_begin = sec.last;
#endif
    // ---- all three histograms from the bytes ------------------------------------------------
    // The sweep counts pass 0's digit only.  The digits of passes 1 and 2 are coarser functions of the same bytes one and
    // two positions earlier, so their histograms are sums of bins of pass 0's, put right at the block's two ends by its
    // first two and last two bytes (sort_bases.h) -- one LDS atomic per position instead of three, and the two that are
    // gone are the ones whose lanes met on few addresses (7-bit digits of Zipf bytes).
    const SortEnds ends = {src[0], src[1], src[bytes - 2], src[bytes - 1]};
    for (int d = tid; d < kSortBins; d += kSortThreads) { lds.gbase[0][d] = 0; }
    __syncthreads();
    // a thread takes four neighbouring positions from two dwords, the next two already in flight; the few positions
    // after the last whole quad (its 7 bytes must exist) go one by one
    auto count_key = [&](uint32_t key) { atomicAdd(&lds.gbase[0][key & m0], 1u); };
    const uint32_t quads = bytes >= 8 ? (uint32_t)((bytes - 8) / 4) + 1u : 0u;
    if ((uint32_t)tid < quads) {
        uint32_t lo = load_u32_unaligned(src + 4u * (uint32_t)tid), hi = load_u32_unaligned(src + 4u * (uint32_t)tid + 4u);
        for (uint32_t q = (uint32_t)tid; q < quads; q += (uint32_t)kSortThreads) {
            const uint64_t eight = ((uint64_t)hi << 32) | lo;
            const uint32_t nq = q + (uint32_t)kSortThreads < quads ? q + (uint32_t)kSortThreads : q;
            lo = load_u32_unaligned(src + 4u * nq); hi = load_u32_unaligned(src + 4u * nq + 4u);
#pragma unroll
            for (int j = 0; j < 4; j++) { count_key(__builtin_bswap32((uint32_t)(eight >> (8 * j))) >> 8); }
        }
    }
    for (uint32_t k = 4u * quads + (uint32_t)tid; k < count; k += (uint32_t)kSortThreads) { count_key(sort_key(src, bytes, k)); }
    __syncthreads();
    sort_bases_derive(lds.gbase[0], lds.gbase[1], lds.gbase[2], small, ends, tid, kSortThreads);
    __syncthreads();
    if (wave < 3) {                                        // exclusive scans: counts -> bases
        uint32_t* const g = lds.gbase[wave];
        const int per = (1 << (wave == 0 ? w0 : wave == 1 ? w1 : w2)) / kWave;     // 16, 4 or 2 digits per lane
        uint32_t sum = 0;
        for (int j = 0; j < per; j++) { sum += g[per * lane + j]; }
        uint32_t excl = wave_scan(sum) - sum;
        for (int j = 0; j < per; j++) { const uint32_t v = g[per * lane + j]; g[per * lane + j] = excl; excl += v; }
    }
    __syncthreads();
    SORT_SEC(sec, 0)

    // pass 0: identity -> A ; pass 1: A -> B ; pass 2: B -> A
    if (small) {
        sort_pass<10, true>(lds, 0, src, bytes, count, carry, pb, pa, sec);
        for (int pass = 1; pass < 3; pass++) {
            sort_pass<7, true>(lds, pass, src, bytes, count, carry, pass == 1 ? pa : pb, pass == 1 ? pb : pa, sec);
        }
    } else {
        for (int pass = 0; pass < 3; pass++) {
            sort_pass<8, false>(lds, pass, src, bytes, count, carry, pass == 1 ? pa : pb, pass == 1 ? pb : pa, sec);
        }
    }
#ifdef SQZ_STATS
    if (tid == 0 && b == 1) {
        printf("sort block 1: cycles %llu: hist %llu; tiles: loads %llu rank %llu scan_a %llu scan_b %llu place %llu copy_out %llu\n",
               (unsigned long long)(sec.last - sec_begin), (unsigned long long)sec.t[0], (unsigned long long)sec.t[1],
               (unsigned long long)sec.t[2], (unsigned long long)sec.t[3], (unsigned long long)sec.t[4],
               (unsigned long long)sec.t[5], (unsigned long long)sec.t[6]);
    }
#endif
}

// ---------------------------------------------------------------------------
// index_match_kernel.  A wave works through its pages (64 consecutive ranks each) with a FIXED number of memory
// operations per page, none of them behind a divergent branch, and with the next pages' loads in flight:
//   * every lane loads S from a clamped rank (the last valid rank again where the page runs over the end), two
//     pages ahead;
//   * every lane loads its position's 16 bytes with one unaligned 16-byte load from min(i, n - 16), one page ahead
//     (as soon as that page's S is there); a position in the stream's last 15 bytes shifts what it got right by
//     i - (n - 16) bytes, zero-filled -- the bytes the stream has from i on, zeros behind its end;
//   * every lane stores its match word; a lane without a rank stores the page's last valid word to that word's
//     position again (as the sort's copy-out does).
// Both loads sit in a register double buffer.  gfx950 counts stores in vmcnt like loads, so a wait for "everything"
// at the top of a page is also a wait for the scattered store of the page before to be acknowledged -- and that
// store is the slowest operation of the kernel.  With the loads issued ahead, what a page's compare needs set out
// BEFORE the store of the page before it: the top of a page waits for nothing, and the one wait of the loop stands
// at the end of a page's compute, in front of the page's own store (as compiled: the `s_waitcnt vmcnt` figures are
// in DESIGN.md section 5).  The first page stands apart from the loop, so that the loop is entered with the same
// operations in flight as its back edge has (the compiler's wait counts are the minimum over both ways in).  Blocks
// shorter than 16 bytes (no 16-byte load fits) are one page of at most 13 positions: its lanes walk by themselves.
struct __attribute__((packed)) U128u { uint32_t w[4]; };

// Section timers of the instrumented build (tools/build_stats.sh): cycles of wave 0 of block 1 per section, summed
// over its pages.  0 the page's positions and bytes have arrived (the instrumented build waits for them there:
// vmcnt(0), which also waits for the store of the page before), 1 candidate loop (shared walk or several runs),
// 2 own walks of the lanes the registers could not settle, 3 store issue.
struct MatchSec {
#ifdef SQZ_STATS
    uint64_t t[4] = {0, 0, 0, 0};
    uint64_t last = 0;
#endif
};
#ifdef SQZ_STATS
#define MATCH_SEC(s, k) SORT_SEC(s, k)
#define MATCH_SEC_LOADS(s, k) SORT_SEC_LOADS(s, k)
#else
#define MATCH_SEC(s, k)
#define MATCH_SEC_LOADS(s, k)
#endif

// bytes k.. of the 16 in w0..w3 move to the front, zeros follow (k = 0..15)
__device__ __forceinline__ void drop_bytes(uint32_t& w0, uint32_t& w1, uint32_t& w2, uint32_t& w3, uint32_t k) {
    uint64_t lo = ((uint64_t)w1 << 32) | w0, hi = ((uint64_t)w3 << 32) | w2;
    const uint32_t s = 8u * k;
    if (s >= 64u) { lo = hi >> (s - 64u); hi = 0; }
    else if (s != 0u) { lo = (lo >> s) | (hi << (64u - s)); hi >>= s; }
    w0 = (uint32_t)lo; w1 = (uint32_t)(lo >> 32); w2 = (uint32_t)hi; w3 = (uint32_t)(hi >> 32);
}

__global__ __launch_bounds__(256)
void index_match_kernel(const uint8_t* __restrict__ in,
                        const uint64_t* __restrict__ in_off,
                        uint32_t n_blocks, uint32_t window,
                        const uint32_t* __restrict__ sorted,
                        uint32_t* __restrict__ match, uint32_t groups, uint64_t slots) {
    // A stream's workgroups all run on ONE XCD, one stream after the other: workgroup k is
    // dispatched to XCD k % 8, so stream b = 8 * (k / 8 / groups) + k % 8.  Its bytes and
    // sorted positions (~1.3 MB for 256 KB) then stay in that XCD's 4 MB L2 while they are
    // gathered at random.  Measured (PMC, 1 GiB batch): FETCH 185 GB with the stream on the
    // fast grid axis, 16.3 GB with consecutive workgroups sharing a stream across all eight
    // L2s, 3.5 GB with this mapping (61 -> 38 ms).  The 4-byte scatter into match[] is NOT
    // helped by it: WRITE_SIZE stayed at 41-47 GB for 4 GB of match words.  Measured ceiling
    // of fixing that: the same kernel storing to match[rank] (contiguous) takes 30 ms.
    const uint32_t xcd = blockIdx.x % (uint32_t)kXcds;
    const uint32_t local = blockIdx.x / (uint32_t)kXcds;
    const uint32_t b = (local / groups) * (uint32_t)kXcds + xcd;
    const uint32_t group = local % groups;
    if (b >= n_blocks || in_off[b + 1] > slots) { return; }
    const uint8_t* src = in + in_off[b];
    const uint64_t bytes = in_off[b + 1] - in_off[b];
    if (bytes < 3) { return; }
    const uint32_t n = (uint32_t)bytes;
    const uint32_t count = n - 2;
    const uint32_t* S = sorted + in_off[b];
    uint32_t* M = match + in_off[b];

    const int lane = (int)(threadIdx.x & (kWave - 1));
    // A wave owns a CONTIGUOUS run of pages (a page = 64 consecutive ranks), so that the page it has just
    // finished is still in its registers when the next one looks back across the page's first rank.
    const uint32_t pages = (count + (uint32_t)kWave - 1u) / (uint32_t)kWave;
    const uint32_t waves = groups * (blockDim.x / (uint32_t)kWave);
    const uint32_t per_wave = (pages + waves - 1u) / waves;
    const uint32_t wave_id = group * (blockDim.x / (uint32_t)kWave) + (threadIdx.x - (uint32_t)lane) / (uint32_t)kWave;
    const uint32_t page_lo = wave_id * per_wave;
    const uint32_t page_hi = page_lo + per_wave < pages ? page_lo + per_wave : pages;
    if (page_lo >= page_hi) { return; }
    MatchSec sec;
#ifdef SQZ_STATS
    sec.last = __builtin_readcyclecounter();
    const uint64_t sec_begin = sec.last;
#endif
    // one lane on its own: the candidates of ranks q_from-1, q_from-2, ... (nearest first).
    // Where the walk ends -- the first rank of the run, or the first candidate within reach, whichever is
    // later -- is found FIRST (ranks are in position order inside a run, so "same key and within reach" is
    // monotone: doubling steps, then bisection), and the lane's own byte at the length to beat is kept in
    // a register: what is left per candidate is its position (neighbouring lanes read neighbouring ranks)
    // and ONE scattered byte, where it used to be three scattered loads.  These walks are gather-bound
    // (executables: a thousand candidates per position).  They are the rare path: their loads wait for everything.
    auto walk = [&](const uint32_t q_from, const uint32_t i, const uint32_t key, const uint32_t cap, const uint32_t reach,
                    uint32_t& best, uint32_t& dist) __attribute__((always_inline)) {
        if (q_from == 0 || best >= cap) { return; }
        auto inside = [&](uint32_t r) {                    // r < q_from <= own rank: S[r] < i when the key is the same
            const uint32_t p = S[r];
            if (p + 4 > n) { return false; }               // (another key's position may end the stream)
            return (load_u32_unaligned(src + p) & 0x00FFFFFFu) == key && i - p <= reach;
        };
        uint32_t q_lo;                                     // candidates are ranks [q_lo, q_from)
        {
            uint32_t d = 4, bad = 0, good = q_from;       // ranks < bad... : `bad - 1` is outside or bad == 0
            bool open = true;
            while (open) {
                if (d >= q_from) { bad = 0; open = false; if (inside(0)) { good = 0; } else { bad = 1; } }
                else if (inside(q_from - d)) { good = q_from - d; d <<= 1; }
                else { bad = q_from - d + 1; open = false; }
            }
            // first inside rank is in [bad, good]
            uint32_t lo = bad, hi = good;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (inside(mid)) { hi = mid; } else { lo = mid + 1; }
            }
            q_lo = lo;
        }
        uint8_t own_next = best >= (uint32_t)kLenMin ? src[i + best] : (uint8_t)0;   // best < cap: i + best < n
        for (uint32_t q = q_from; q > q_lo && best < cap; ) {
            q--;
            const uint32_t p = S[q];
            if (best >= (uint32_t)kLenMin && src[p + best] != own_next) { continue; }
            uint32_t k = 3;
            while (k < cap) {
                if (i + k + 4 <= n) {
                    const uint32_t x = load_u32_unaligned(src + p + k) ^ load_u32_unaligned(src + i + k);
                    if (x != 0) { k += (uint32_t)__builtin_ctz(x) >> 3; break; }
                    k += 4;
                } else {
                    if (src[p + k] != src[i + k]) { break; }
                    k++;
                }
            }
            if (k > cap) { k = cap; }
            if (k > best) {                                // strictly longer: nearest among equals
                best = k; dist = i - p;
                if (best < cap) { own_next = src[i + best]; }
            }
        }
    };
    if (n < 16u) {
        // ---- a block shorter than 16 bytes: at most 13 positions, one page, and no room for a 16-byte load ----
        // (block-uniform, outside the page pipeline)  Every lane walks its own run, which is the same search.
        if ((uint32_t)lane < count) {
            const uint32_t i = S[lane];
            const uint32_t key = (uint32_t)src[i] | ((uint32_t)src[i + 1] << 8) | ((uint32_t)src[i + 2] << 16);   // i <= n - 3
            const uint32_t cap = n - i;
            const uint32_t reach = i < window - 1 ? i : window - 1;
            uint32_t best = 0, dist = 0;
            walk((uint32_t)lane, i, key, cap, reach, best, dist);
            M[i] = best >= (uint32_t)kLenMin ? ((best << 16) | dist) : (key & 0xFFu);
        }
        return;
    }
    const uint32_t tail = n - 16u;                           // the last position a 16-byte load may start at
    const uint32_t page_last = page_hi - 1u;
    // the S value of this lane's rank in page pg: a page behind the wave's last one is the last one again, a rank
    // behind the stream's last one is the last one again -- always a load, always inside S[0, count)
    auto fetch_pos = [&](uint32_t pg) {
        const uint32_t r = (pg < page_last ? pg : page_last) * (uint32_t)kWave + (uint32_t)lane;
        return S[r < count - 1u ? r : count - 1u];
    };
    auto fetch16 = [&](uint32_t at) { return *reinterpret_cast<const U128u*>(src + (at < tail ? at : tail)); };
    // what fetch16(at) brought, as the 16 bytes from `at` on (zeros beyond the stream's end: never compared, lengths
    // stop at cap <= n - i).  Only the stream's last 15 positions have anything to do here.
    auto settle16 = [&](uint32_t at, const U128u& got, uint32_t& w0, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
        w0 = got.w[0]; w1 = got.w[1]; w2 = got.w[2]; w3 = got.w[3];
        if (__ballot(at > tail) != 0) { drop_bytes(w0, w1, w2, w3, at > tail ? at - tail : 0u); }
    };
    // the page in front of the current one: positions and their first 16 bytes (lane = rank inside the page)
    uint32_t prev_i = 0, prev0 = 0, prev1 = 0, prev2 = 0, prev3 = 0;

    // ---- one page: position i and its bytes are in registers ---------------------------------------------
    auto do_page = [&](const uint32_t pg, const uint32_t i, const uint32_t own0, const uint32_t own1,
                       const uint32_t own2, const uint32_t own3) __attribute__((always_inline)) {
        MATCH_SEC_LOADS(sec, 0)
        const uint32_t r0 = pg * (uint32_t)kWave;
        const bool have_prev = pg > 0;
        const uint32_t r = r0 + (uint32_t)lane;              // a wave owns 64 consecutive ranks
        const bool valid = r < count;                        // (a lane without a rank holds the last rank's position)
        const uint32_t cap = (n - i) < (uint32_t)kLenMax ? (n - i) : (uint32_t)kLenMax;
        const uint32_t reach = i < window - 1 ? i : window - 1;
        const uint32_t key = own0 & 0x00FFFFFFu;             // i <= n - 3: the key's bytes are the stream's
        uint32_t best = 0, dist = 0;
        bool later = false;                                  // this lane finishes by itself, from rank `resume` down
        uint32_t resume = 0;
        const uint32_t key0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
        if (__ballot(valid && key == key0 && i <= tail) == ~0ull) {
            // ---- the whole wave sits inside one run of equal keys (a frequent 3-byte string) ---
            // Its lanes walk the same candidates, one rank apart.  Walk them ONCE: every lane compares the
            // candidate with its own first 16 bytes, held in registers.  Same order (nearest first), same strict >.
            bool alive = true;
            // page = sorted positions of ranks [page_base, +64) AND their first 16 bytes, one rank per lane: a
            // candidate's position and bytes come out of these registers (v_readlane) -- one gather per 64
            // candidates instead of a dependent load per candidate (each turn of this loop used to wait for it)
            uint32_t page_base = r0, page = i, pb0 = own0, pb1 = own1, pb2 = own2, pb3 = own3;
            const uint64_t own_lo = ((uint64_t)own1 << 32) | own0, own_hi = ((uint64_t)own3 << 32) | own2;
            for (int64_t c = (int64_t)r0 + kWave - 2; c >= 0; c--) {
                if (c < (int64_t)page_base) {
                    page_base -= (uint32_t)kWave;            // r0 is a multiple of 64: so is every page
                    page = S[page_base + (uint32_t)lane];    // (every rank of an earlier page exists)
                    settle16(page, fetch16(page), pb0, pb1, pb2, pb3);
                }
                const int at = (int)(c - (int64_t)page_base);
                const uint32_t pc = (uint32_t)__builtin_amdgcn_readlane((int)page, at);
                const bool below = (int64_t)r > c;           // the candidate comes before my position
                const uint32_t d = i - pc;
                alive &= !(below & (d > reach));             // everything further is farther
                if (__ballot(alive) == 0) { break; }
                // its key first: a rank in front of the run can be any position
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)pb0, at);
                if ((c0 & 0x00FFFFFFu) != key0) { break; }   // left the run: so have all earlier ranks
                const uint32_t c1 = (uint32_t)__builtin_amdgcn_readlane((int)pb1, at);
                const uint32_t c2 = (uint32_t)__builtin_amdgcn_readlane((int)pb2, at);
                const uint32_t c3 = (uint32_t)__builtin_amdgcn_readlane((int)pb3, at);
                const uint64_t x_lo = own_lo ^ (((uint64_t)c1 << 32) | c0), x_hi = own_hi ^ (((uint64_t)c3 << 32) | c2);
                uint32_t len = x_lo != 0 ? ((uint32_t)__builtin_ctzll(x_lo) >> 3)
                             : x_hi != 0 ? 8u + ((uint32_t)__builtin_ctzll(x_hi) >> 3) : 16u;
                const bool want = below & alive;
                // longer than the registers hold: this lane goes on by itself from here (a long compare inside
                // this loop would hold up the other 63 lanes)
                const bool full = want & (len == 16u) & (cap > 16u);
                later |= full;
                resume = full ? (uint32_t)c + 1u : resume;
                alive &= !full;
                len = len > cap ? cap : len;
                const bool better = want & !full & (len > best);     // strictly longer: nearest among equals
                best = better ? len : best;
                dist = better ? d : dist;
                alive &= best < cap;
                // a run of long matches (padding, repeated records): nearly every lane ends up on
                // its own anyway, so stop sharing early instead of trickling them out one per turn
                if (__builtin_popcountll(__ballot(later)) >= kSharedGiveUp) {
                    if (alive) {
                        later = true;
                        resume = below ? (uint32_t)c : r;    // ranks [c, r) are behind me / nothing is
                    }
                    break;
                }
            }
        } else {
            // ---- several runs in one wave (the usual case: 2.7 candidates per position on Zipf bytes) ------
            // The candidates of rank r are the ranks r-1, r-2, ... of its run, nearest first -- and those are
            // the positions the NEIGHBOURING LANES hold, in this page or in the one before it (kept from the
            // previous turn of the loop).  A candidate's position and bytes come out of lane l-k's registers
            // through the LDS crossbar (ds_bpermute): no gather and no dependent load per candidate (a lane that
            // walks by itself pays three dependent global loads per candidate, and one such lane holds up its
            // wave: with per-lane walks the kernel ran at 13 us per page).  Same order, same strict >.  What the
            // registers cannot settle leaves the loop and is finished by the lane itself with walk(): a match
            // longer than the 16 bytes held, and a run that reaches back more than 64 ranks.
            // A turn is branch-free but for three wave-uniform branches: the lane's state is ONE predicate,
            // `alive`, that conditions are and-ed into, and every update is a select.
            bool alive = valid;
            const uint64_t own_lo = ((uint64_t)own1 << 32) | own0;
            for (int k = 1; k <= kWave; k++) {
                const int from = lane - k;
                const bool in_cur = from >= 0;
                alive &= in_cur | have_prev;                         // nothing lies in front of rank 0
                if (__ballot(alive) == 0) { break; }
                const int addr = (from & (kWave - 1)) << 2;
                uint32_t pc = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)i);
                uint32_t c0 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)own0);
                uint32_t c1 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)own1);
                const bool back = __ballot(alive & !in_cur) != 0;    // someone looks into the page before
                if (back) {
                    const uint32_t qc = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)prev_i);
                    const uint32_t q0 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)prev0);
                    const uint32_t q1 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)prev1);
                    pc = in_cur ? pc : qc; c0 = in_cur ? c0 : q0; c1 = in_cur ? c1 : q1;
                }
                const uint64_t x = own_lo ^ (((uint64_t)c1 << 32) | c0);
                const uint32_t d = i - pc;
                // left the run (so have all earlier ranks) or out of reach (everything further is farther)
                alive &= (((uint32_t)x & 0x00FFFFFFu) == 0u) & (d <= reach);
                uint32_t len = x != 0 ? ((uint32_t)__builtin_ctzll(x) >> 3) : 8u;
                if (__ballot(alive & (len == 8u) & (cap > 8u)) != 0) {      // (rare on Zipf bytes: the other two words)
                    uint32_t c2 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)own2);
                    uint32_t c3 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)own3);
                    if (back) {
                        const uint32_t q2 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)prev2);
                        const uint32_t q3 = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)prev3);
                        c2 = in_cur ? c2 : q2; c3 = in_cur ? c3 : q3;
                    }
                    const uint64_t x_hi = (((uint64_t)own3 << 32) | own2) ^ (((uint64_t)c3 << 32) | c2);
                    const uint32_t more = x_hi != 0 ? 8u + ((uint32_t)__builtin_ctzll(x_hi) >> 3) : 16u;
                    len = len == 8u ? more : len;
                }
                // longer than the registers hold: this lane goes on by itself, starting with this very candidate
                const bool full = alive & (len == 16u) & (cap > 16u);
                later |= full;
                resume = full ? r - (uint32_t)k + 1u : resume;
                alive &= !full;
                len = len > cap ? cap : len;
                const bool better = alive & (len > best);            // strictly longer: nearest among equals
                best = better ? len : best;
                dist = better ? d : dist;
                alive &= best < cap;
            }
            // (the loop ran out with the lane still looking) 64 ranks back and still inside the run
            resume = alive ? r - (uint32_t)kWave : resume;
            later |= alive;
        }
        MATCH_SEC(sec, 1)
        if (later) { walk(resume, i, key, cap, reach, best, dist); }
        MATCH_SEC(sec, 2)
        // no match: the literal itself.  A lane without a rank holds the last rank's position: it stores that
        // rank's word there again.
        const uint32_t word = best >= (uint32_t)kLenMin ? ((best << 16) | dist) : (key & 0xFFu);
        const uint32_t ranks = count - r0;                   // of this page, if fewer than 64
        const uint32_t last_word = (uint32_t)__builtin_amdgcn_readlane((int)word, (int)(ranks < (uint32_t)kWave ? ranks - 1u : (uint32_t)kWave - 1u));
        M[i] = valid ? word : last_word;
        MATCH_SEC(sec, 3)
        prev_i = i; prev0 = own0; prev1 = own1; prev2 = own2; prev3 = own3;
    };

    // ---- the pipeline: positions two pages ahead, bytes one page ahead ---------------------------------------
    uint32_t pos_cur = fetch_pos(page_lo);
    uint32_t pos_nxt = fetch_pos(page_lo + 1u);
    if (page_lo > 0) {                                       // (every rank of an earlier page exists)
        prev_i = S[(page_lo - 1u) * (uint32_t)kWave + (uint32_t)lane];
        settle16(prev_i, fetch16(prev_i), prev0, prev1, prev2, prev3);
    }
    U128u got_cur = fetch16(pos_cur);
    {   // the first page, apart from the loop: nothing of a page before it is in flight
        const uint32_t pos_far = fetch_pos(page_lo + 2u);
        const U128u got_nxt = fetch16(pos_nxt);
        uint32_t own0, own1, own2, own3;
        settle16(pos_cur, got_cur, own0, own1, own2, own3);
        do_page(page_lo, pos_cur, own0, own1, own2, own3);
        pos_cur = pos_nxt; pos_nxt = pos_far; got_cur = got_nxt;
    }
    for (uint32_t pg = page_lo + 1u; pg < page_hi; pg++) {
        // in flight here, oldest first: pos_nxt (page pg + 1), got_cur (page pg), the store of page pg - 1
        const uint32_t pos_far = fetch_pos(pg + 2u);
        const U128u got_nxt = fetch16(pos_nxt);              // waits for pos_nxt: two operations behind it
        uint32_t own0, own1, own2, own3;
        settle16(pos_cur, got_cur, own0, own1, own2, own3);  // waits for got_cur: three operations behind it
        do_page(pg, pos_cur, own0, own1, own2, own3);
        pos_cur = pos_nxt; pos_nxt = pos_far; got_cur = got_nxt;
    }
#ifdef SQZ_STATS
    if (threadIdx.x == 0 && b == 1 && group == 0) {
        printf("match block 1: cycles %llu: loads %llu candidates %llu own_walks %llu store %llu\n",
               (unsigned long long)(sec.last - sec_begin), (unsigned long long)sec.t[0], (unsigned long long)sec.t[1],
               (unsigned long long)sec.t[2], (unsigned long long)sec.t[3]);
    }
#endif
}

// ---------------------------------------------------------------------------
// Greedy parse (squeeze.h:377-394) over the match table, without the serial walk.
// Token starts are the positions reachable from 0 through next(i) = i + (match ? len : 1).
// A tile of 64 chunks is staged in LDS; lane l first walks chunk l from its first position
// on its own (a guess: the real way in is not known yet).  Two walks that ever land on the
// same position are the same from there on, so the real path through a chunk -- entered
// where the previous chunk's path left -- only has to be followed until it steps on a
// position the guess also visited; from there the guess is right.  That fix-up runs chunk
// by chunk, a few hops each, instead of one hop per token.
//
// No memory round trip stands in a tile's way: its 32 rows of match words are loaded back to back
// into registers while the tile before is walked, and its token words, packed in LDS, leave in 32
// stores of 64 consecutive words that nothing waits for.  (One load, one wait, one LDS write, 32
// times per tile, behind the lane-strided token stores of the tile before, was 60 % of the kernel.)
constexpr int kChunk = 32;                          // positions per lane (<= 32: one mask bit each)
constexpr int kTile = kChunk * kWave;               // positions per pass
constexpr int kChunkRow = kChunk + 1;               // padded: same-offset reads of all lanes spread over the banks

// 8,448 B per stream: 16 streams per CU, the whole 4096-block batch in one round (with the tile's
// bytes staged as well it was 10,496 B, 15 per CU and two rounds: 9.9 ms instead of 5).  The
// literal travels in the match word instead: len << 16 | dist for a match (len >= 3), the byte
// itself (len field 0) where index_match_kernel found none.  Once every lane has taken its chunk's
// words into registers the same words hold the tile's token words, token n at m[n] (unpadded), on
// their way out.
struct ParseLds {
    uint32_t m[kChunkRow * kWave];                  // match word per position (row l = chunk l, padded); then the tile's token words
};

__device__ __forceinline__ uint32_t parse_slot(uint32_t k) { return k + (k / (uint32_t)kChunk); }

// how far a token reaches: its match length, 1 for a literal.  Match words come from
// index_match_kernel (length >= 3); the floor of 1 is there so that the walks below end
// whatever the table holds -- a word with a zero length field must not stall a wave.
__device__ __forceinline__ uint32_t parse_step(uint32_t w) {
    const uint32_t len = w >> 16;
    return len != 0 ? len : 1u;
}

// The one-step lazy rule: a match gives way to a literal where the very next position holds a longer one
// (w1 = the successor's word; a literal's length field is 0, so a successor without a match never wins).
// The decision depends on the position alone, so the walks below stay walks of a step function.
__device__ __forceinline__ bool lazy_defers(uint32_t w, uint32_t w1) {
    const uint32_t len = w >> 16;
    return len >= (uint32_t)kLenMin && (w1 >> 16) > len;
}

// A tile's match words as they travel: lane l holds positions l, l + 64, ... of the tile, one coalesced load each,
// all issued back to back.  Positions past the stream's end read its last word again (clamped, never used).
constexpr int kTileRows = kTile / kWave;
__device__ __forceinline__ void parse_fetch(uint32_t (&w)[kTileRows], const uint32_t* __restrict__ M,
                                            const uint64_t tile, const uint64_t bytes, const int lane) {
    const uint64_t left = bytes - tile;
    const uint32_t last = left < (uint64_t)kTile ? (uint32_t)left - 1u : (uint32_t)kTile - 1u;
    const uint32_t* __restrict__ T = M + tile;
#pragma unroll
    for (int j = 0; j < kTileRows; j++) {
        const uint32_t k = (uint32_t)(j * kWave + lane);
        w[j] = T[k < last ? k : last];
    }
}

// A value the compiler must work out again in every tile: without it the lane's 32 slot numbers of an unrolled
// loop are kept in 32 registers across the tiles, and the kernel no longer fits 4 waves per SIMD.
__device__ __forceinline__ uint32_t per_tile(uint32_t v) {
#ifndef SQZ_WAVE_EMU
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// Section timers of the instrumented build (tools/build_stats.sh): cycles of block 1 per section, summed over its
// tiles.  0 the tile's words have arrived (the instrumented build waits for them there: vmcnt(0), which also waits
// for the token stores of the tile before), 1 stage to LDS and send for the next tile, 2 guess walk, 3 fix-up
// across the 64 chunks, 4 token write (pack in LDS, issue the stores).
struct ParseSec {
#ifdef SQZ_STATS
    uint64_t t[5] = {0, 0, 0, 0, 0};
    uint64_t last = 0;
#endif
};
#ifdef SQZ_STATS
#define PARSE_SEC(s, k) SORT_SEC(s, k)
#define PARSE_SEC_LOADS(s, k) SORT_SEC_LOADS(s, k)
#else
#define PARSE_SEC(s, k)
#define PARSE_SEC_LOADS(s, k)
#endif

// kLazy = false is the greedy parse, the reference's (and, instruction for instruction, the kernel this was before it
// became a template); kLazy = true applies lazy_defers() on top of it.  The decision at a position depends on that
// position alone, so the scheme stands: every lane first turns its chunk's words into a mask of the positions that
// give way (`defer`), and the guess walks and the fix-up step by 1 where the mask says so.  The lazy instantiation
// needs two things the greedy one does not:
//   * the successor's word at every position.  Inside a chunk it is the next word of the row; at a chunk's last
//     position it is the first word of the next lane's row, read straight from there; at the tile's last position
//     it is the first word of the NEXT tile: one more load (33 per tile) that travels with the tile's own 32, a
//     tile ahead like them.  Position bytes-2, and everything behind it, is a literal: nothing gives way to it.
//   * the byte of a token start that gives way (a match word does not carry it).  These are a few per cent of the
//     tokens, and the tile's bytes neither fit the LDS (8,448 B are what 16 streams per CU leave) nor the
//     registers (8 words per lane held across the tile: 147 VGPRs).  After the fix-up every lane sends for the
//     bytes of the first two such tokens of its chunk -- always two loads -- and writes them over the match
//     tokens once those are packed in LDS; a chunk with more than two fetches the rest one by one.  The wait for
//     them is a wait for loads that set out after the next tile's words and before this tile's token stores: it
//     never waits for the stores, and the next tile's words have had the walks' time to arrive.
//
// gfx950, -Rpass-analysis=kernel-resource-usage: greedy 117 VGPRs, lazy 125; no scratch, no spills; 8,448 B of LDS
// both.  The 4 waves per SIMD = 16 streams per CU that the LDS admits need <= 128.
template <bool kLazy>
__global__ __launch_bounds__(kWave)
void index_parse_kernel(const uint8_t* __restrict__ in,
                        const uint64_t* __restrict__ in_off,
                        uint32_t n_blocks,
                        const uint32_t* __restrict__ match,
                        uint32_t* __restrict__ tokens,
                        uint32_t* __restrict__ tok_count, uint64_t slots) {
    __shared__ ParseLds lds;
    const uint32_t b = blockIdx.x;
    if (b >= n_blocks) { return; }
    const int lane = threadIdx.x;
    if (in_off[b + 1] > slots) {                  // the caller's arrays do not reach this far: refuse the block
        if (lane == 0) { tok_count[b] = kRefused; }
        return;
    }
    const uint8_t* src = in + in_off[b];
    const uint64_t bytes = in_off[b + 1] - in_off[b];
    const uint32_t* M = match + in_off[b];
    uint32_t* tok = tokens + in_off[b];

    if (bytes == 0) {
        if (lane == 0) { tok_count[b] = 0; }
        return;
    }
    // positions bytes-2, bytes-1 have no 3-byte prefix and no match word: literals
    const uint32_t lit1 = (uint32_t)src[bytes - 1];
    const uint32_t lit2 = (uint32_t)src[bytes >= 2 ? bytes - 2 : 0];

    ParseSec sec;
#ifdef SQZ_STATS
    sec.last = __builtin_readcyclecounter();
    const uint64_t sec_begin = sec.last;
#endif
    uint32_t ntok = 0;
    uint32_t entry = 0;                              // where the real path enters the tile (tile-relative)
    uint32_t fly[kTileRows];                         // the tile in flight
    parse_fetch(fly, M, 0, bytes, lane);
    uint32_t fly_next = 0;                           // lazy: the first word of the tile behind the one in flight
    // (the index goes through a vector register: the word comes by the same road as the others and is counted with them)
    auto fetch_next = [&](const uint64_t tile) __attribute__((always_inline)) {
        const uint64_t at = tile + (uint64_t)per_tile((uint32_t)kTile);
        fly_next = M[at < bytes ? at : bytes - 1];
    };
    if constexpr (kLazy) { fetch_next(0); }
    // one tile; false: the path has left the stream (its last token reaches over the ragged last tile)
    auto do_tile = [&](const uint64_t tile) __attribute__((always_inline)) -> bool {
        const uint64_t left = bytes - tile;
        const uint32_t have = left < (uint64_t)kTile ? (uint32_t)left : (uint32_t)kTile;
        if (entry >= have) { return false; }
        PARSE_SEC_LOADS(sec, 0)
        lds_barrier();                               // the tile before has been copied out of lds.m
        const int t2 = left < (uint64_t)(kTile + 2) ? (int)left - 2 : kTile;     // tile-relative: position bytes-2
        uint32_t* const mine_at = &lds.m[parse_slot((uint32_t)lane)];
#pragma unroll
        for (int j = 0; j < kTileRows; j++) {        // position j * kWave + lane: a row of 64 lies 64 + 64 / kChunk slots behind the row before
            const int tj = t2 - j * kWave;
            mine_at[j * (kWave + kWave / kChunk)] = lane < tj ? fly[j] : lane == tj ? lit2 : lit1;
        }
        uint32_t over = 0;                           // lazy: the word behind the tile's last one, if that position can hold a match at all
        if constexpr (kLazy) {
            over = left > (uint64_t)(kTile + 2) ? fly_next : 0u;
        }
        lds_barrier();
        // the next tile's words set out now and are taken up after this tile's tokens have left (behind the
        // last tile: the same tile once more, into registers nobody reads)
        const uint64_t ahead = tile + (uint64_t)kTile < bytes ? tile + (uint64_t)kTile : tile;
        parse_fetch(fly, M, ahead, bytes, lane);
        if constexpr (kLazy) { fetch_next(ahead); }
        PARSE_SEC(sec, 1)

        // ---- every lane: its chunk from the chunk's first position ---------------------
        const uint32_t lo = (uint32_t)lane * (uint32_t)kChunk;
        const uint32_t room = have > lo ? (have - lo < (uint32_t)kChunk ? have - lo : (uint32_t)kChunk) : 0u;
        const uint32_t* row = &lds.m[lane * kChunkRow];
        uint32_t defer = 0;                          // lazy: one bit per position of the chunk that gives way to its successor
        if constexpr (kLazy) {                       // (a loop, eight words at a time: unrolled it holds the row in registers)
            // the successor of the chunk's last word: the first word of the next lane's row, of the next tile for lane 63
            const uint32_t behind = lane + 1 < kWave ? lds.m[(lane + 1 < kWave ? lane + 1 : lane) * kChunkRow] : over;
            uint32_t w = row[0];
#pragma unroll 1
            for (int j0 = 0; j0 < kChunk; j0 += 8) {
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const uint32_t w1 = j0 + j + 1 < kChunk ? row[j0 + j + 1] : behind;
                    defer |= (lazy_defers(w, w1) ? 1u : 0u) << (j0 + j);
                    w = w1;
                }
            }
        }
        uint32_t guess = 0;                          // one bit per position of the chunk (kChunk <= 32)
        uint32_t p = 0;
        while (p < room) {
            guess |= 1u << p;
            const uint32_t w = row[p];
            if constexpr (kLazy) { p += ((defer >> p) & 1u) != 0 ? 1u : parse_step(w); } else { p += parse_step(w); }
        }
        const uint32_t guess_out = lo + p;           // where the guess leaves the chunk (>= lo + room)
        PARSE_SEC(sec, 2)

        // ---- the real path, chunk by chunk (uniform) -----------------------------------
        // One turn per chunk the path enters (a long token takes it straight to the chunk it lands in).  Where
        // the path enters on a position the guess visited -- most chunks -- the turn is two lane reads and a
        // handful of scalar instructions; otherwise it hops through LDS until it meets the guess or leaves the
        // chunk.  A lane only notes where its chunk's real path meets its guess (`from`) and the token starts in
        // front of that (`extra`); the bitmaps are put together by all lanes at once afterwards.
        uint32_t extra = 0;
        uint32_t from = (uint32_t)kChunk;            // kChunk: the path never meets this lane's guess
        uint32_t e = entry;
        while (e < have) {
            const uint32_t l = e / (uint32_t)kChunk;
            const uint32_t clo = l * (uint32_t)kChunk;
            const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)guess, (int)l);
            uint32_t q = e - clo;
            if (((g >> q) & 1u) != 0) {              // the guess was here too: the rest of the chunk is the guess's
                e = (uint32_t)__builtin_amdgcn_readlane((int)guess_out, (int)l);
                if ((uint32_t)lane == l) { from = q; }
                continue;
            }
            const uint32_t croom = have - clo < (uint32_t)kChunk ? have - clo : (uint32_t)kChunk;
            uint32_t real = 0;
            do {                                     // it was not: hop
                real |= 1u << q;
                const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds.m[l * kChunkRow + q]);
                if constexpr (kLazy) {
                    const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)defer, (int)l);
                    q += ((dl >> q) & 1u) != 0 ? 1u : parse_step(w);
                } else {
                    q += parse_step(w);
                }
            } while (q < croom && ((g >> q) & 1u) == 0);
            const bool met = q < croom;              // on a position of the guess (which has none at or beyond croom)
            e = met ? (uint32_t)__builtin_amdgcn_readlane((int)guess_out, (int)l) : clo + q;
            if ((uint32_t)lane == l) { extra = real; from = met ? q : (uint32_t)kChunk; }
        }
        const uint32_t mine = extra | (from < (uint32_t)kChunk ? guess & (~0u << from) : 0u);   // this lane's chunk: real token starts
        entry = e - (uint32_t)kTile;                 // e >= have here; carried into the next tile
        // lazy: the token starts that give way are literals of their bytes, which no match word carries.  They are a
        // few per cent of the tokens: every lane sends for the first two of its chunk here -- always two loads, so
        // that the waits stay counted ones -- and writes them over the match tokens further down; a chunk with more
        // (rare) fetches the rest there, one by one.
        uint32_t give = 0, give_j0 = 0, give_j1 = 0, give_b0 = 0, give_b1 = 0;
        if constexpr (kLazy) {
            give = mine & defer;
            const uint32_t second = give & (give - 1u);
            give_j0 = give != 0 ? (uint32_t)__builtin_ctz(give) : 0u;
            give_j1 = second != 0 ? (uint32_t)__builtin_ctz(second) : give_j0;
            const uint64_t at0 = tile + (uint64_t)(lo + give_j0), at1 = tile + (uint64_t)(lo + give_j1);
            give_b0 = src[at0 < bytes ? at0 : bytes - 1];        // (a lane without any reads a byte it does not use)
            give_b1 = src[at1 < bytes ? at1 : bytes - 1];
        }
        PARSE_SEC(sec, 3)

        // ---- token words, in order ----------------------------------------------------
        // Every lane takes its chunk's words into registers; from then on the tile's match words are dead, and
        // the token words are packed into the same LDS, token n of the tile at word n (no padding).  They leave
        // 64 consecutive words per store, always kTileRows stores: the ones past the tile's last token write
        // that last token again.  A fixed number of stores lets the wait for the next tile's words, which set
        // out before them, count the stores off instead of waiting for them.
        uint32_t mw[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; j++) { mw[j] = row[j]; }
        const uint32_t cnt = (uint32_t)__builtin_popcount(mine);
        const uint32_t incl = wave_scan(cnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);   // >= 1: entry < have
        lds_barrier();
        uint32_t at = incl - cnt;
#pragma unroll
        for (int j = 0; j < kChunk; j++) {
            if ((mine >> j) & 1u) {
                lds.m[at++] = (mw[j] >> 16) != 0 ? (kTokMatch | mw[j]) : (mw[j] & 0xFFu);
            }
        }
        if constexpr (kLazy) {                       // token n of the chunk is the n-th set bit of `mine`
            const uint32_t first = incl - cnt;
            auto slot_of = [&](uint32_t j) { return first + (uint32_t)__builtin_popcount(mine & ((1u << j) - 1u)); };
            uint32_t rest = give;
            if (rest != 0) { lds.m[slot_of(give_j0)] = give_b0; rest &= rest - 1u; }
            if (rest != 0) { lds.m[slot_of(give_j1)] = give_b1; rest &= rest - 1u; }
            while (rest != 0) {
                const uint32_t j = (uint32_t)__builtin_ctz(rest);
                rest &= rest - 1u;
                lds.m[slot_of(j)] = (uint32_t)src[tile + (uint64_t)(lo + j)];
            }
        }
        lds_barrier();
        uint32_t* const out = tok + ntok;
        const uint32_t last = total - 1u;
        const uint32_t ln = per_tile((uint32_t)lane);
#pragma unroll
        for (int j = 0; j < kTileRows; j++) {
            const uint32_t k = (uint32_t)(j * kWave) + ln;
            const uint32_t n = (k < last ? k : last) & (uint32_t)(kTile - 1);      // (the mask: a 32-bit offset for the store)
            out[n] = lds.m[n];
        }
        ntok += total;
        PARSE_SEC(sec, 4)
        return true;
    };
    // The first tile stands apart from the loop: in the loop a tile's words are always kTileRows loads followed
    // by kTileRows stores away, and the compiler's s_waitcnt vmcnt counts exactly that; merged with the way in
    // from the first fetch (no stores behind it) it would have to wait for the stores as well.
    static_assert(kTile > kLenMax, "a token never reaches over a whole tile");
    if (do_tile(0)) {
        for (uint64_t tile = (uint64_t)kTile; tile < bytes; tile += (uint64_t)kTile) {
            if (!do_tile(tile)) { break; }
        }
    }
    if (lane == 0) { tok_count[b] = ntok; }
#ifdef SQZ_STATS
    if (lane == 0 && b == 1) {
        printf("parse block 1: cycles %llu: tiles: arrived %llu stage %llu guess %llu fixup %llu write %llu\n",
               (unsigned long long)(sec.last - sec_begin), (unsigned long long)sec.t[0], (unsigned long long)sec.t[1],
               (unsigned long long)sec.t[2], (unsigned long long)sec.t[3], (unsigned long long)sec.t[4]);
    }
#endif
}

// ---------------------------------------------------------------------------
// Shared dictionary (SQZF version 3): the longest match whose source STARTS in the dictionary, merged into the
// match table index_match_kernel left.  A block under a dictionary Dct is coded as the bytes Dct || B from
// position D = len(Dct) on, so a dictionary position q is the candidate at distance D - q + i of block position
// i: every in-block candidate is nearer than every dictionary candidate, and the dictionary's match replaces the
// table's only when it is STRICTLY longer (nearest among equals).  Dictionary candidates nearest first:
// q = D-1 and q = D-2, whose 3-byte prefix runs on into the block and therefore has no entry in the index, then
// the run of the index with the position's own prefix from its highest position down.  A source that starts in
// the dictionary runs on into the block (Dct[D-1] is followed by B[0]), and may run on over position i itself.
//
// One workgroup holds the dictionary (at most 32,767 bytes) and its sorted positions (16 bits each, at most
// 64 KB) in LDS, loaded once with 16-byte loads, and then works through blocks blockIdx.x, + gridDim.x, ...:
// one thread per position.  A position finds both ends of its prefix's run by two bisections over the sorted
// positions (15 steps of two LDS reads each); every candidate compare reads the dictionary from LDS, four bytes at a time;
// only the position's own bytes (consecutive threads, consecutive bytes) and a source's tail inside the block
// come from memory.  Positions i >= window - 1 cannot reach the dictionary and are not visited.
#ifndef SQZ_DICT_THREADS
#define SQZ_DICT_THREADS 1024                     // (the CPU wave emulator of tests/emu runs workgroups of up to 8 waves)
#endif
constexpr int kDictThreads = SQZ_DICT_THREADS;
struct DictLds {
    uint8_t byte[kMaxWindow];                    // the dictionary, zeros behind its end
    uint16_t rank[kMaxWindow];                   // positions 0 .. D-3 by 3-byte prefix, ascending inside a run
};                                               // 96 KB: one workgroup (16 waves) per CU

__global__ __launch_bounds__(kDictThreads)
void dict_match_kernel(const uint8_t* __restrict__ in,
                       const uint64_t* __restrict__ in_off,
                       uint32_t n_blocks, uint32_t window,
                       const uint8_t* __restrict__ dict, uint32_t D,
                       const uint32_t* __restrict__ dsorted,      // index_sort_kernel's result for the dictionary
                       uint32_t* __restrict__ match, uint64_t slots) {
    __shared__ __attribute__((aligned(16))) DictLds lds;
    const uint32_t tid = threadIdx.x;
    if (D == 0 || D >= (uint32_t)kMaxWindow) { return; }          // (the callers refuse these)
    const uint32_t cnt = D >= 3 ? D - 2 : 0u;                     // positions with an entry in the index
    {
        // the dictionary: whole 16-byte groups where its address allows them, bytes otherwise; zeros to the end
        const bool aligned = (reinterpret_cast<uintptr_t>(dict) & 15u) == 0;
        const uint32_t groups = aligned ? D / 16u : 0u;
        for (uint32_t g = tid; g < groups; g += (uint32_t)kDictThreads) {
            reinterpret_cast<uint4*>(lds.byte)[g] = reinterpret_cast<const uint4*>(dict)[g];
        }
        for (uint32_t k = groups * 16u + tid; k < (uint32_t)kMaxWindow; k += (uint32_t)kDictThreads) {
            lds.byte[k] = k < D ? dict[k] : (uint8_t)0;
        }
        // the sorted positions: four 32-bit words in, four 16-bit values out (the array is the sort's: 256-byte
        // aligned, D + 64 slots; what lies behind cnt is never looked at)
        const uint32_t quads = (cnt + 3u) / 4u;
        for (uint32_t g = tid; g < quads; g += (uint32_t)kDictThreads) {
            const uint4 v = reinterpret_cast<const uint4*>(dsorted)[g];
            SortCntPair* const two = reinterpret_cast<SortCntPair*>(lds.rank) + 2u * g;   // two 16-bit values per word
            two[0] = (v.x & 0xFFFFu) | (v.y << 16);
            two[1] = (v.z & 0xFFFFu) | (v.w << 16);
        }
    }
    __syncthreads();
    auto lds_u32 = [&](uint32_t at) { return reinterpret_cast<const U32u*>(lds.byte + at)->v; };   // at + 4 <= 32768
    auto dkey = [&](uint32_t p) { return __builtin_bswap32(lds_u32(p)) >> 8; };                     // p <= D - 3
    const uint32_t reach = window - 1u;

    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        if (in_off[b + 1] > slots) { continue; }                  // beyond the caller's arrays: index_parse refuses the block
        const uint8_t* src = in + in_off[b];
        const uint64_t bytes = in_off[b + 1] - in_off[b];
        if (bytes < 3) { continue; }
        uint32_t* M = match + in_off[b];
        // positions with a table word (the last two have none) that can reach Dct[D-1]: i + 1 <= window - 1
        const uint64_t upto = bytes - 2 < (uint64_t)reach ? bytes - 2 : (uint64_t)reach;
        for (uint32_t i = tid; i < (uint32_t)upto; i += (uint32_t)kDictThreads) {
            const uint64_t left = bytes - i;
            const uint32_t cap = left < (uint64_t)kLenMax ? (uint32_t)left : (uint32_t)kLenMax;
            uint32_t best = M[i] >> 16;                           // the in-block match to beat (0: a literal)
            if (best >= cap) { continue; }
            const uint32_t q_min = D + i > reach ? D + i - reach : 0u;   // the farthest dictionary position within reach
            // byte v of Dct || B
            auto vbyte = [&](uint32_t v) { return v < D ? lds.byte[v] : src[v - D]; };
            // how far Dct || B at q agrees with B at i, up to cap
            auto extend = [&](uint32_t q) {
                const uint32_t in_d = D - q < cap ? D - q : cap;  // the part of the source inside the dictionary
                uint32_t k = 0;
                while (k < in_d) {
                    if (k + 4 <= in_d) {                          // (k + 4 <= cap <= bytes - i: the own dword exists)
                        const uint32_t x = lds_u32(q + k) ^ load_u32_unaligned(src + i + k);
                        if (x != 0) { return k + ((uint32_t)__builtin_ctz(x) >> 3); }
                        k += 4;
                    } else {
                        if (lds.byte[q + k] != src[i + k]) { return k; }
                        k++;
                    }
                }
                while (k < cap) {                                 // on into the block: source byte q + k - D < k
                    const uint32_t s = q + k - D;
                    if (k + 4 <= cap) {
                        const uint32_t x = load_u32_unaligned(src + s) ^ load_u32_unaligned(src + i + k);
                        if (x != 0) { return k + ((uint32_t)__builtin_ctz(x) >> 3); }
                        k += 4;
                    } else {
                        if (src[s] != src[i + k]) { return k; }
                        k++;
                    }
                }
                return k;
            };
            uint32_t dist = 0;
            uint8_t own_next = best >= (uint32_t)kLenMin ? src[i + best] : (uint8_t)0;     // best < cap: i + best < bytes
            auto consider = [&](uint32_t q) {
                if (best >= (uint32_t)kLenMin && vbyte(q + best) != own_next) { return; }  // cannot be longer
                const uint32_t len = extend(q);
                if (len >= (uint32_t)kLenMin && len > best) {     // strictly longer: nearest among equals
                    best = len; dist = D + i - q;
                    if (best < cap) { own_next = src[i + best]; }
                }
            };
            if (D - 1u >= q_min) { consider(D - 1u); }
            if (D >= 2u && D - 2u >= q_min && best < cap) { consider(D - 2u); }
            if (cnt != 0 && best < cap) {
                const uint32_t key = sort_key(src, bytes, i);     // i <= bytes - 3
                uint32_t lo = 0, hi = cnt;                        // `end`: the first rank whose key is greater than mine
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (dkey(lds.rank[mid]) <= key) { lo = mid + 1; } else { hi = mid; }
                }
                uint32_t end = lo;
                lo = 0; hi = end;                                 // `begin`: the first rank whose key is mine (end: none)
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (dkey(lds.rank[mid]) < key) { lo = mid + 1; } else { hi = mid; }
                }
                const uint32_t begin = lo;
                while (end > begin && best < cap) {               // the run, nearest first: no prefix to look at again
                    const uint32_t q = lds.rank[--end];
                    if (q < q_min) { break; }                     // everything further is farther
                    consider(q);
                }
            }
            if (dist != 0) { M[i] = (best << 16) | dist; }
        }
    }
}

void launch_index_sort(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                       uint32_t* buf_a, uint32_t* buf_b, uint64_t slots,
                       hipStream_t stream) {
    if (n_blocks == 0) { return; }
    hipLaunchKernelGGL(index_sort_kernel, dim3(n_blocks), dim3(kSortThreads), 0, stream,
                       in, in_off, n_blocks, buf_a, buf_b, slots);
}

void launch_index_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                        uint32_t window, const uint32_t* sorted, uint32_t* match,
                        uint32_t match_groups, uint64_t slots, hipStream_t stream) {
    if (n_blocks == 0) { return; }
    if (match_groups < 1) { match_groups = 1; }
    const uint32_t rounded = (n_blocks + (uint32_t)kXcds - 1) / (uint32_t)kXcds * (uint32_t)kXcds;
    while ((uint64_t)match_groups * rounded > 0x7FFFFFFFull) { match_groups = (match_groups + 1) / 2; }
    hipLaunchKernelGGL(index_match_kernel, dim3(rounded * match_groups), dim3(256), 0, stream,
                       in, in_off, n_blocks, window, sorted, match, match_groups, slots);
}

void launch_index_parse(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                        const uint32_t* match, uint32_t* tokens, uint32_t* tok_count,
                        uint64_t slots, hipStream_t stream) {
    if (n_blocks == 0) { return; }
    hipLaunchKernelGGL(index_parse_kernel<false>, dim3(n_blocks), dim3(kWave), 0, stream,
                       in, in_off, n_blocks, match, tokens, tok_count, slots);
}

void launch_index_parse_lazy(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks,
                             const uint32_t* match, uint32_t* tokens, uint32_t* tok_count,
                             uint64_t slots, hipStream_t stream) {
    if (n_blocks == 0) { return; }
    hipLaunchKernelGGL(index_parse_kernel<true>, dim3(n_blocks), dim3(kWave), 0, stream,
                       in, in_off, n_blocks, match, tokens, tok_count, slots);
}

void launch_dict_match(const uint8_t* in, const uint64_t* in_off, uint32_t n_blocks, uint32_t window,
                       const uint8_t* dict, uint32_t dict_bytes, const uint32_t* dict_sorted,
                       uint32_t* match, uint64_t slots, hipStream_t stream) {
    if (n_blocks == 0) { return; }
    const uint32_t grid = n_blocks < 1024u ? n_blocks : 1024u;  // a workgroup loads the dictionary once and takes every grid-th block
    hipLaunchKernelGGL(dict_match_kernel, dim3(grid), dim3(kDictThreads), 0, stream,
                       in, in_off, n_blocks, window, dict, dict_bytes, dict_sorted, match, slots);
}

} // namespace sqzk
