// sqz_amd/csrc/shuffle.hip -- the byte-shuffle filter of SQZF version 4 on the device (gfx950).
// Format and rule: include/sqz/sqz.h, DESIGN.md section 10, "Version 4".
//
// Range b is the L = off[b + 1] - off[b] bytes at off[b], in the source and in the destination alike; with
// e = elem_bytes and m = L / e (rounded down) the forward transform writes
//     S[j * m + i] = B[i * e + j]      0 <= i < m, 0 <= j < e
// plane after plane, and leaves the L - m * e tail bytes where they were, behind the planes; the inverse undoes it.
// Source and destination must not overlap.  Nothing is assumed about alignment -- of the base pointers, of off[b]
// or of the plane bases j * m -- and nothing outside a range is read or written.
//
// A memory-bound transposition, built like range_copy_kernel (frame.hip).  `groups` workgroups share a range tile
// by tile; a tile is kShufTile bytes of the range, kShufTile / e elements.  Both sides of a tile are cut into
// 16-byte rows on ADDRESS boundaries: a row that lies whole inside the range is one aligned 16-byte load, a row
// that lies whole inside the tile's part of a plane (forward) or of the elements (inverse) is one aligned 16-byte
// store, the bytes in front of the first and behind the last such row go singly.  Between the two sides the tile
// lies in LDS as it was loaded -- a loaded row at its own place, so that neither side's alignment reaches the
// other's -- and the store side picks its 16 bytes out of it one by one (ds_read_u8).
//
// The LDS image (bank of a byte address a: (a / 4) % 32 for ds_write_b32 and the narrow reads, conflicts counted
// within each half of a wave):
//   forward   the tile's source bytes in their order.  Lane l of a half gathers destination row r0 + l of one
//             plane: at step k it reads byte 16 e (r0 + l) + e k + j, 4 e dwords from its neighbour's -- 8, 16 or
//             32 banks apart, an 8-, 16- or 32-way conflict.  One dword of padding behind every 16 e bytes makes
//             that 4 e + 1, which is odd: 32 lanes, 32 banks.
//   inverse   e plane images, each the tile's part of a plane in its order.  Lane l gathers destination row r0 + l
//             of the elements: at step k all lanes read the same plane, 16 / e bytes from their neighbour's.  For
//             e = 4 that is one dword and for e = 8 half a dword (two lanes share a dword: a broadcast), both free
//             of conflicts as they are; for e = 2 it is two dwords (lanes l and l + 16 meet), and one dword of
//             padding behind every 128 bytes of a plane image sends the upper 16 lanes to the odd banks.
//   the row-wise side (both directions) writes a loaded row as four dwords.  Neighbouring lanes' rows are 4 dwords
//   apart, which would be a 4-way conflict; every group of 8 lanes therefore starts at another of its four dwords,
//   and the four groups of a half cover all 32 banks at every step.
//
// Two kernels: shuffle_blocks_kernel<E, kInverse> with one element size for the launch, and shuffle_ranges_kernel
// <kInverse> with one per range (a batch of frames, frame.hip: every frame has its own), where 0 copies the range as
// it is, so that a mixed batch goes through one pass into one buffer.  The second dispatches once per range into
// shuffle_range_body<E, kInverse>, which is shuffle_blocks_kernel's per-range code word for word.  It is a COPY:
// calling the body from shuffle_blocks_kernel as well moved that kernel's registers (e = 8 forward: 60 -> 72 VGPRs,
// occupancy 8 -> 7), so the older kernel keeps its own text.  A change to one belongs in both.
#include "sqz_kernels.h"

namespace sqzk {

namespace {

constexpr int kShufThreads = 256;
constexpr uint32_t kShufTile = 8192;               // bytes of a range per tile: two 16-byte rows a lane on either side
// the image: the tile, the bytes of its first and last row that lie outside it, and the padding
constexpr uint32_t kShufLdsBytes = kShufTile + 8 * 32 + 4 * (kShufTile / 32 + 16) + 64;

constexpr uint32_t shuf_log2(uint32_t e) { return e == 2 ? 1u : e == 4 ? 2u : 3u; }

// where byte x of the forward image lies: one dword more behind every 16 e bytes
template <uint32_t E>
__device__ __forceinline__ uint32_t fwd_at(uint32_t x) { return x + 4u * (x >> (4u + shuf_log2(E))); }
// where byte p of a plane image lies (inverse): one dword more behind every 128 bytes for e = 2
template <uint32_t E>
__device__ __forceinline__ uint32_t inv_at(uint32_t p) { return E == 2 ? p + 4u * (p >> 7) : p; }
// bytes between two plane images: the tile's part of a plane, a row's slack at either end, the padding; whole rows
template <uint32_t E>
constexpr uint32_t inv_plane_stride() {
    const uint32_t t = kShufTile / E + 32;
    return ((E == 2 ? t + 4u * (t >> 7) : t) + 15u) & ~15u;
}
static_assert(kShufTile + 32 + 4 * ((kShufTile + 32) / 32 + 1) <= kShufLdsBytes, "the forward image fits");
static_assert(2 * inv_plane_stride<2>() <= kShufLdsBytes && 4 * inv_plane_stride<4>() <= kShufLdsBytes &&
              8 * inv_plane_stride<8>() <= kShufLdsBytes, "the plane images fit");

// the 16-byte row at `row` (16-byte aligned): one aligned load when it lies whole inside [lo, hi), else its bytes
// inside [lo, hi) singly and zeros for the others
__device__ __forceinline__ uint4 shuf_load_row(const uint8_t* row, const uint8_t* lo, const uint8_t* hi) {
    if (row >= lo && row + 16 <= hi) { return *reinterpret_cast<const uint4*>(row); }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        if (row + k >= lo && row + k < hi) { w[k >> 2] |= (uint32_t)row[k] << (8 * (k & 3)); }
    }
    uint4 r;
    r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
    return r;
}

// a loaded row into the image at dword `at`, every group of 8 lanes starting at another of the four dwords
__device__ __forceinline__ void shuf_put_row(uint32_t* lds, uint32_t at, const uint4& v, uint32_t tid) {
    const uint32_t rot = (tid >> 3) & 3u;
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t w = (s + rot) & 3u;
        lds[at + w] = w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w;
    }
}

__device__ __forceinline__ uint4 shuf_pack(const uint32_t (&b)[16]) {
    uint4 v;
    v.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    v.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    v.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    v.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
    return v;
}

// One range for workgroup g of the `groups` that share it tile by tile: the bytes [o0, o1) of src and of dst alike,
// through the image `lds` (kShufLdsBytes).  kInverse = false: dst range = the shuffle of src range; true: the other way.
template <uint32_t E, bool kInverse>
__device__ __forceinline__
void shuffle_range_body(uint32_t* lds, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t o0,
                        uint64_t o1, uint32_t g, uint32_t groups) {
    constexpr uint32_t kLog = shuf_log2(E);
    constexpr uint32_t T = kShufTile / E;          // elements of a tile
    constexpr uint32_t kRows = T / 16;             // full rows of a tile's part of a plane at the most
    const uint64_t len = o1 > o0 ? o1 - o0 : 0;
    const uint64_t m = len >> kLog;
    const uint8_t* const from = src + o0;
    const uint8_t* const from_end = from + len;
    uint8_t* const to = dst + o0;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const ldsb = reinterpret_cast<const uint8_t*>(lds);
    if (g == 0) {                                  // the tail bytes keep their place
        const uint64_t at = m << kLog;
        if (tid < len - at) { to[at + tid] = from[at + tid]; }
    }
    const uint64_t tiles = (m + T - 1) / T;
    for (uint64_t tile = g; tile < tiles; tile += groups) {        // (the same trips for every lane of the workgroup)
        const uint64_t i0 = tile * T;
        const uint32_t cnt = m - i0 < T ? (uint32_t)(m - i0) : T;  // elements of this tile
        if constexpr (!kInverse) {
            // ---- load: the tile's source bytes, rows on address boundaries, each at its own place in the image
            const uint8_t* const a0 = from + (i0 << kLog);
            const uint32_t nb = cnt << kLog;
            const uint32_t h = (uint32_t)((uintptr_t)a0 & 15u);
            const uint8_t* const base = a0 - h;
            const uint32_t rows = (h + nb + 15u) / 16u;
            for (uint32_t r = tid; r < rows; r += kShufThreads) {
                const uint4 v = shuf_load_row(base + 16 * r, from, from_end);
                shuf_put_row(lds, fwd_at<E>(16 * r) >> 2, v, tid);
            }
            __syncthreads();
            // ---- store: plane by plane, full rows of the destination; byte 16 k' + .. of plane j is element's byte j
            const uint32_t m15 = (uint32_t)(m & 15u), t15 = (uint32_t)(((uintptr_t)to + i0) & 15u);
            for (uint32_t w = tid; w < E * kRows; w += kShufThreads) {
                const uint32_t j = w / kRows, r = w % kRows;
                const uint32_t d15 = (t15 + j * m15) & 15u;        // the plane part's first byte within its row
                uint32_t hd = (16u - d15) & 15u;
                if (hd > cnt) { hd = cnt; }
                if (r < (cnt - hd) / 16u) {
                    const uint32_t idx = hd + 16u * r;             // the row's first element within the tile
                    const uint32_t y0 = h + (idx << kLog) + j;
                    const uint32_t pad0 = y0 >> (4u + kLog);       // a row's 16 e bytes cross one padding dword at most
                    const uint32_t edge = (pad0 + 1u) << (4u + kLog);
                    const uint8_t* const p = ldsb + y0 + 4u * pad0;
                    uint32_t bytes[16];
#pragma unroll
                    for (uint32_t k = 0; k < 16; k++) { bytes[k] = p[E * k + (y0 + E * k >= edge ? 4u : 0u)]; }
                    *reinterpret_cast<uint4*>(to + (uint64_t)j * m + i0 + idx) = shuf_pack(bytes);
                }
            }
            // the bytes in front of the first and behind the last full row of every plane part: 32 lanes a plane
            {
                const uint32_t j = tid >> 5, q = tid & 31u;
                if (j < E) {
                    const uint32_t d15 = (t15 + j * m15) & 15u;
                    uint32_t hd = (16u - d15) & 15u;
                    if (hd > cnt) { hd = cnt; }
                    const uint32_t full = (cnt - hd) / 16u, tl = cnt - hd - 16u * full;
                    uint32_t idx = 0xFFFFFFFFu;
                    if (q < hd) { idx = q; } else if (q >= 16 && q - 16 < tl) { idx = hd + 16u * full + (q - 16); }
                    if (idx != 0xFFFFFFFFu) {
                        to[(uint64_t)j * m + i0 + idx] = ldsb[fwd_at<E>(h + (idx << kLog) + j)];
                    }
                }
            }
        } else {
            constexpr uint32_t PS = inv_plane_stride<E>();
            // ---- load: the tile's part of every plane, rows on address boundaries, into that plane's image
            const uint32_t m15 = (uint32_t)(m & 15u), f15 = (uint32_t)(((uintptr_t)from + i0) & 15u);
            for (uint32_t w = tid; w < E * (kRows + 1); w += kShufThreads) {
                const uint32_t j = w / (kRows + 1), r = w % (kRows + 1);
                const uint32_t h = (f15 + j * m15) & 15u;
                if (16u * r < h + cnt) {
                    const uint8_t* const base = from + (uint64_t)j * m + i0 - h;
                    const uint4 v = shuf_load_row(base + 16 * r, from, from_end);
                    shuf_put_row(lds, (j * PS + inv_at<E>(16 * r)) >> 2, v, tid);
                }
            }
            __syncthreads();
            // ---- store: the tile's elements, full rows of the destination; byte x of it is byte x % e of element x / e
            uint8_t* const d0 = to + (i0 << kLog);
            const uint32_t nb = cnt << kLog;
            uint32_t hd = (16u - (uint32_t)((uintptr_t)d0 & 15u)) & 15u;
            if (hd > nb) { hd = nb; }
            const uint32_t full = (nb - hd) / 16u, tl = nb - hd - 16u * full;
            for (uint32_t r = tid; r < full; r += kShufThreads) {
                const uint32_t x0 = hd + 16u * r;
                uint32_t bytes[16];
#pragma unroll
                for (uint32_t k = 0; k < 16; k++) {
                    const uint32_t j = (hd + k) & (E - 1u);        // the same plane for every lane: 16 r is whole elements
                    const uint32_t h = (f15 + j * m15) & 15u;
                    bytes[k] = ldsb[j * PS + inv_at<E>(h + ((x0 + k) >> kLog))];
                }
                *reinterpret_cast<uint4*>(d0 + x0) = shuf_pack(bytes);
            }
            {
                uint32_t x = 0xFFFFFFFFu;
                if (tid < hd) { x = tid; } else if (tid >= 32 && tid - 32 < tl) { x = hd + 16u * full + (tid - 32); }
                if (x != 0xFFFFFFFFu) {
                    const uint32_t j = x & (E - 1u);
                    const uint32_t h = (f15 + j * m15) & 15u;
                    d0[x] = ldsb[j * PS + inv_at<E>(h + (x >> kLog))];
                }
            }
        }
        __syncthreads();                           // the image is read: the next tile may take its place
    }
}

// bytes s .. s + 7 of lo:hi
__device__ __forceinline__ uint64_t shuf_join_bytes(uint64_t lo, uint64_t hi, uint32_t s) {
    return s == 0 ? lo : (lo >> (8 * s)) | (hi << (64 - 8 * s));
}

// The same range copied as it is, by the same row rules and without the image: the destination's full 16-byte rows
// are aligned stores, a row's source bytes one aligned load where both sides share the alignment, two aligned loads
// joined by a byte shift where they do not and both lie whole inside the range, single bytes otherwise; the bytes in
// front of the first and behind the last full row go singly.  The workgroups share the range tile by tile.
__device__ __forceinline__
void shuffle_copy_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t o0, uint64_t o1,
                       uint32_t g, uint32_t groups) {
    constexpr uint32_t kTileRows = kShufTile / 16;
    const uint64_t len = o1 > o0 ? o1 - o0 : 0;
    const uint8_t* const from = src + o0;
    const uint8_t* const from_end = from + len;
    uint8_t* const to = dst + o0;
    const uint32_t tid = threadIdx.x;
    uint64_t head = (16u - (uint32_t)((uintptr_t)to & 15u)) & 15u;
    if (head > len) { head = len; }
    const uint64_t rows = (len - head) / 16;
    const uint64_t tail_at = head + 16 * rows;
    if (g == 0) {
        if (tid < head) { to[tid] = from[tid]; }
        if (tid >= 32 && tid - 32 < len - tail_at) { to[tail_at + (tid - 32)] = from[tail_at + (tid - 32)]; }
    }
    const uint8_t* const fb = from + head;
    uint8_t* const tb = to + head;                 // 16-byte aligned
    const uint32_t sh = (uint32_t)((uintptr_t)fb & 15u);
    const uint64_t tiles = (rows + kTileRows - 1) / kTileRows;
    for (uint64_t tile = g; tile < tiles; tile += groups) {
        const uint64_t r1 = (tile + 1) * kTileRows < rows ? (tile + 1) * kTileRows : rows;
        for (uint64_t k = tile * kTileRows + tid; k < r1; k += kShufThreads) {
            const uint8_t* const sp = fb + 16 * k;
            uint4 v;
            if (sh == 0) {
                v = *reinterpret_cast<const uint4*>(sp);
            } else if (sp - sh >= from && sp - sh + 32 <= from_end) {
                const uint4 a = *reinterpret_cast<const uint4*>(sp - sh);
                const uint4 c = *reinterpret_cast<const uint4*>(sp - sh + 16);
                const uint64_t q0 = (uint64_t)a.x | ((uint64_t)a.y << 32), q1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
                const uint64_t q2 = (uint64_t)c.x | ((uint64_t)c.y << 32), q3 = (uint64_t)c.z | ((uint64_t)c.w << 32);
                const bool up = sh >= 8;
                const uint32_t s = sh & 7u;
                const uint64_t lo = shuf_join_bytes(up ? q1 : q0, up ? q2 : q1, s);
                const uint64_t hi = shuf_join_bytes(up ? q2 : q1, up ? q3 : q2, s);
                v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};  // a source row that is not whole inside the range: byte by byte
#pragma unroll
                for (uint32_t j = 0; j < 16; j++) { w[j >> 2] |= (uint32_t)sp[j] << (8 * (j & 3)); }
                v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
            }
            *reinterpret_cast<uint4*>(tb + 16 * k) = v;
        }
    }
}

} // namespace

// kInverse = false: dst range = the shuffle of src range; true: the other way.  skip: ranges with skip[b] != 0 are
// left alone (null: none is).  `groups` workgroups share a range tile by tile.
template <uint32_t E, bool kInverse>
__global__ __launch_bounds__(kShufThreads)
void shuffle_blocks_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                           const uint64_t* __restrict__ off, const uint32_t* __restrict__ skip, uint32_t n_ranges,
                           uint32_t groups) {
    __shared__ uint32_t lds[kShufLdsBytes / 4];
    constexpr uint32_t kLog = shuf_log2(E);
    constexpr uint32_t T = kShufTile / E;          // elements of a tile
    constexpr uint32_t kRows = T / 16;             // full rows of a tile's part of a plane at the most
    const uint32_t b = blockIdx.x / groups, g = blockIdx.x % groups;
    if (b >= n_ranges) { return; }
    if (skip != nullptr && skip[b] != 0) { return; }
    const uint64_t o0 = off[b], o1 = off[b + 1];
    const uint64_t len = o1 > o0 ? o1 - o0 : 0;
    const uint64_t m = len >> kLog;
    const uint8_t* const from = src + o0;
    const uint8_t* const from_end = from + len;
    uint8_t* const to = dst + o0;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const ldsb = reinterpret_cast<const uint8_t*>(lds);
    if (g == 0) {                                  // the tail bytes keep their place
        const uint64_t at = m << kLog;
        if (tid < len - at) { to[at + tid] = from[at + tid]; }
    }
    const uint64_t tiles = (m + T - 1) / T;
    for (uint64_t tile = g; tile < tiles; tile += groups) {        // (the same trips for every lane of the workgroup)
        const uint64_t i0 = tile * T;
        const uint32_t cnt = m - i0 < T ? (uint32_t)(m - i0) : T;  // elements of this tile
        if constexpr (!kInverse) {
            // ---- load: the tile's source bytes, rows on address boundaries, each at its own place in the image
            const uint8_t* const a0 = from + (i0 << kLog);
            const uint32_t nb = cnt << kLog;
            const uint32_t h = (uint32_t)((uintptr_t)a0 & 15u);
            const uint8_t* const base = a0 - h;
            const uint32_t rows = (h + nb + 15u) / 16u;
            for (uint32_t r = tid; r < rows; r += kShufThreads) {
                const uint4 v = shuf_load_row(base + 16 * r, from, from_end);
                shuf_put_row(lds, fwd_at<E>(16 * r) >> 2, v, tid);
            }
            __syncthreads();
            // ---- store: plane by plane, full rows of the destination; byte 16 k' + .. of plane j is element's byte j
            const uint32_t m15 = (uint32_t)(m & 15u), t15 = (uint32_t)(((uintptr_t)to + i0) & 15u);
            for (uint32_t w = tid; w < E * kRows; w += kShufThreads) {
                const uint32_t j = w / kRows, r = w % kRows;
                const uint32_t d15 = (t15 + j * m15) & 15u;        // the plane part's first byte within its row
                uint32_t hd = (16u - d15) & 15u;
                if (hd > cnt) { hd = cnt; }
                if (r < (cnt - hd) / 16u) {
                    const uint32_t idx = hd + 16u * r;             // the row's first element within the tile
                    const uint32_t y0 = h + (idx << kLog) + j;
                    const uint32_t pad0 = y0 >> (4u + kLog);       // a row's 16 e bytes cross one padding dword at most
                    const uint32_t edge = (pad0 + 1u) << (4u + kLog);
                    const uint8_t* const p = ldsb + y0 + 4u * pad0;
                    uint32_t bytes[16];
#pragma unroll
                    for (uint32_t k = 0; k < 16; k++) { bytes[k] = p[E * k + (y0 + E * k >= edge ? 4u : 0u)]; }
                    *reinterpret_cast<uint4*>(to + (uint64_t)j * m + i0 + idx) = shuf_pack(bytes);
                }
            }
            // the bytes in front of the first and behind the last full row of every plane part: 32 lanes a plane
            {
                const uint32_t j = tid >> 5, q = tid & 31u;
                if (j < E) {
                    const uint32_t d15 = (t15 + j * m15) & 15u;
                    uint32_t hd = (16u - d15) & 15u;
                    if (hd > cnt) { hd = cnt; }
                    const uint32_t full = (cnt - hd) / 16u, tl = cnt - hd - 16u * full;
                    uint32_t idx = 0xFFFFFFFFu;
                    if (q < hd) { idx = q; } else if (q >= 16 && q - 16 < tl) { idx = hd + 16u * full + (q - 16); }
                    if (idx != 0xFFFFFFFFu) {
                        to[(uint64_t)j * m + i0 + idx] = ldsb[fwd_at<E>(h + (idx << kLog) + j)];
                    }
                }
            }
        } else {
            constexpr uint32_t PS = inv_plane_stride<E>();
            // ---- load: the tile's part of every plane, rows on address boundaries, into that plane's image
            const uint32_t m15 = (uint32_t)(m & 15u), f15 = (uint32_t)(((uintptr_t)from + i0) & 15u);
            for (uint32_t w = tid; w < E * (kRows + 1); w += kShufThreads) {
                const uint32_t j = w / (kRows + 1), r = w % (kRows + 1);
                const uint32_t h = (f15 + j * m15) & 15u;
                if (16u * r < h + cnt) {
                    const uint8_t* const base = from + (uint64_t)j * m + i0 - h;
                    const uint4 v = shuf_load_row(base + 16 * r, from, from_end);
                    shuf_put_row(lds, (j * PS + inv_at<E>(16 * r)) >> 2, v, tid);
                }
            }
            __syncthreads();
            // ---- store: the tile's elements, full rows of the destination; byte x of it is byte x % e of element x / e
            uint8_t* const d0 = to + (i0 << kLog);
            const uint32_t nb = cnt << kLog;
            uint32_t hd = (16u - (uint32_t)((uintptr_t)d0 & 15u)) & 15u;
            if (hd > nb) { hd = nb; }
            const uint32_t full = (nb - hd) / 16u, tl = nb - hd - 16u * full;
            for (uint32_t r = tid; r < full; r += kShufThreads) {
                const uint32_t x0 = hd + 16u * r;
                uint32_t bytes[16];
#pragma unroll
                for (uint32_t k = 0; k < 16; k++) {
                    const uint32_t j = (hd + k) & (E - 1u);        // the same plane for every lane: 16 r is whole elements
                    const uint32_t h = (f15 + j * m15) & 15u;
                    bytes[k] = ldsb[j * PS + inv_at<E>(h + ((x0 + k) >> kLog))];
                }
                *reinterpret_cast<uint4*>(d0 + x0) = shuf_pack(bytes);
            }
            {
                uint32_t x = 0xFFFFFFFFu;
                if (tid < hd) { x = tid; } else if (tid >= 32 && tid - 32 < tl) { x = hd + 16u * full + (tid - 32); }
                if (x != 0xFFFFFFFFu) {
                    const uint32_t j = x & (E - 1u);
                    const uint32_t h = (f15 + j * m15) & 15u;
                    d0[x] = ldsb[j * PS + inv_at<E>(h + (x >> kLog))];
                }
            }
        }
        __syncthreads();                           // the image is read: the next tile may take its place
    }
}

// Ranges of mixed element size in one launch: elem[b] = 2, 4 or 8 is shuffle_blocks_kernel<elem[b]> on range b, 0 copies
// the range as it is; any other value, like skip[b] != 0, leaves it alone.  The element size is uniform for a workgroup:
// one dispatch per range, outside the tile loop, into the bodies above.
template <bool kInverse>
__global__ __launch_bounds__(kShufThreads)
void shuffle_ranges_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                           const uint64_t* __restrict__ off, const uint32_t* __restrict__ skip,
                           const uint32_t* __restrict__ elem, uint32_t n_ranges, uint32_t groups) {
    __shared__ uint32_t lds[kShufLdsBytes / 4];
    const uint32_t b = blockIdx.x / groups, g = blockIdx.x % groups;
    if (b >= n_ranges) { return; }
    if (skip != nullptr && skip[b] != 0) { return; }
    const uint32_t e = elem[b];
    const uint64_t o0 = off[b], o1 = off[b + 1];
    if (e == 0) { shuffle_copy_body(src, dst, o0, o1, g, groups); }
    else if (e == 2) { shuffle_range_body<2, kInverse>(lds, src, dst, o0, o1, g, groups); }
    else if (e == 4) { shuffle_range_body<4, kInverse>(lds, src, dst, o0, o1, g, groups); }
    else if (e == 8) { shuffle_range_body<8, kInverse>(lds, src, dst, o0, o1, g, groups); }
}

// one workgroup per 32 KB of a range, about 8192 workgroups at the most (launch_range_copy's shape); the workgroups
// of a range that is left out, or is shorter than the hint, leave at once
static uint64_t shuffle_groups(uint32_t n_ranges, uint64_t size_hint) {
    uint64_t groups = size_hint != 0 ? (size_hint + 32767) / 32768 : 512;
    const uint64_t cap = 8192 / n_ranges > 1 ? 8192 / n_ranges : 1;
    if (groups > cap) { groups = cap; }
    if (groups > 2048) { groups = 2048; }
    if (groups < 1) { groups = 1; }
    while (groups > 1 && groups * n_ranges > 0x7FFFFFFFull) { groups /= 2; }
    return groups;
}

void launch_shuffle_blocks(const uint8_t* src, const uint64_t* off, uint32_t n_ranges, uint32_t elem_bytes,
                           bool inverse, uint8_t* dst, const uint32_t* skip, uint64_t size_hint, hipStream_t stream) {
    if (n_ranges == 0) { return; }
    const uint64_t groups = shuffle_groups(n_ranges, size_hint);
    const dim3 grid((unsigned)(groups * n_ranges)), block(kShufThreads);
#define SQZ_SHUF_LAUNCH(E, INV) \
    hipLaunchKernelGGL((shuffle_blocks_kernel<E, INV>), grid, block, 0, stream, src, dst, off, skip, n_ranges, (uint32_t)groups)
    if (elem_bytes == 2) { if (inverse) { SQZ_SHUF_LAUNCH(2, true); } else { SQZ_SHUF_LAUNCH(2, false); } }
    else if (elem_bytes == 4) { if (inverse) { SQZ_SHUF_LAUNCH(4, true); } else { SQZ_SHUF_LAUNCH(4, false); } }
    else if (elem_bytes == 8) { if (inverse) { SQZ_SHUF_LAUNCH(8, true); } else { SQZ_SHUF_LAUNCH(8, false); } }
#undef SQZ_SHUF_LAUNCH
}

void launch_shuffle_ranges(const uint8_t* src, const uint64_t* off, const uint32_t* elem, uint32_t n_ranges,
                           bool inverse, uint8_t* dst, const uint32_t* skip, uint64_t size_hint, hipStream_t stream) {
    if (n_ranges == 0) { return; }
    const uint64_t groups = shuffle_groups(n_ranges, size_hint);
    const dim3 grid((unsigned)(groups * n_ranges)), block(kShufThreads);
    if (inverse) {
        hipLaunchKernelGGL(shuffle_ranges_kernel<true>, grid, block, 0, stream, src, dst, off, skip, elem, n_ranges,
                           (uint32_t)groups);
    } else {
        hipLaunchKernelGGL(shuffle_ranges_kernel<false>, grid, block, 0, stream, src, dst, off, skip, elem, n_ranges,
                           (uint32_t)groups);
    }
}

} // namespace sqzk
