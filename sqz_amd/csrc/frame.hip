// sqz_amd/csrc/frame.hip -- the SQZF frame container on the device (gfx950): content checksums,
// index construction (encode) and index validation (decode).  Format: include/sqz/sqz.h, DESIGN.md section 10.
//
// CRC-32 as zlib.crc32 computes it (IEEE 802.3, reflected polynomial 0xEDB88320, initial value and final
// xor 0xFFFFFFFF).  CRC is serial in its textbook form; here it is split by linearity.  With r(M) the
// register after feeding M from state 0 without the final xor,
//     r(A || B) = r(A) * x^(8|B|)  ^  r(B)                 (products of reflected residues mod P)
//     crc(M)    = r(M) ^ 0xFFFFFFFF * x^(8|M|) ^ 0xFFFFFFFF
// and zero bytes IN FRONT of a message leave r unchanged.  crc32_blocks_kernel cuts a byte range into
// 64-byte chunks on 16-byte ADDRESS boundaries (so every full row is one aligned 16-byte load; the
// bytes of the first row that lie before the range count as zeros, which is free), lane t of a
// 256-lane workgroup reduces chunks t, t + 256, ... and carries them forward with the compile-time
// multiplier x^(8 * 16384), the lanes are brought to a common end with a 256-entry table of x^(512 d),
// xor-reduced, and the ragged last chunk (1..64 bytes, reduced byte-exactly by the lane that owns it)
// is appended.  A long range is shared by several workgroups: each adds its part, moved to the end of
// the range by x^(8 * bytes behind it), with an atomic xor.
//
// The per-chunk reduction is the table-free bitwise loop: three vector operations per message bit on gfx950
// (v_bfe_i32, v_lshrrev_b32, v_bitop3_b32), no LDS and no table traffic, so the kernel is bound by
// instruction issue, not by HBM.  Slicing tables in LDS would trade those for one 4-byte LDS read per byte
// at data-dependent addresses; they were not built: DESIGN.md section 10 has the measured time of this form
// against the encode step it rides on.
#include "sqz_kernels.h"

namespace sqzk {

namespace {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;          // x^0 in the reflected representation
constexpr int kCrcThreads = 256;
constexpr uint32_t kChunk = 64;                    // bytes a lane reduces at a time: four 16-byte rows
constexpr uint64_t kMinPart = 16384;               // a workgroup's share of a range: at least one tile

constexpr int kErrEINVAL = 22, kErrE2BIG = 7, kErrEILSEQ = 84;     // <errno.h>, checked in abi.hip

// a * b mod P, both reflected residues: 32 shift-and-xor steps (constexpr: host, device and tables)
constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & kCrcPoly);
    }
    return p;
}

struct CrcTables {
    uint32_t pow2[32];     // x^(2^k); x^(2^32 - 1) = 1, so x^(2^(k + 32)) = x^(2^k)
    uint32_t m512[256];    // x^(512 d): the bits of d chunks
};
constexpr CrcTables make_crc_tables() {
    CrcTables t{};
    uint32_t p = kCrcOne >> 1;                     // x^1
    t.pow2[0] = p;
    for (int k = 1; k < 32; k++) { p = gf_mul(p, p); t.pow2[k] = p; }
    uint32_t m = kCrcOne;
    for (int d = 0; d < 256; d++) { t.m512[d] = m; m = gf_mul(m, t.pow2[9]); }
    return t;
}
constexpr CrcTables kCrcTablesValue = make_crc_tables();
constexpr uint32_t kTileMul = kCrcTablesValue.pow2[17];            // x^(8 * 256 * 64): one tile of chunks further
__device__ const CrcTables kCrcTab = kCrcTablesValue;

// a * K for a compile-time K: after unrolling every K * x^i is a constant, three operations per bit of a
template <uint32_t K>
__device__ __forceinline__ uint32_t gf_mul_const(uint32_t a) {
    uint32_t p = 0, b = K;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & kCrcPoly);
    }
    return p;
}

// the register after `bits` more message bits whose values were xored into its low end already
__device__ __forceinline__ uint32_t crc_shift(uint32_t c, int bits) {
    for (int k = 0; k < bits; k++) { c = (c >> 1) ^ ((0u - (c & 1u)) & kCrcPoly); }
    return c;
}
__device__ __forceinline__ uint32_t crc_word(uint32_t c) {         // four message bytes (little-endian word)
#pragma unroll
    for (int k = 0; k < 32; k++) { c = (c >> 1) ^ ((0u - (c & 1u)) & kCrcPoly); }
    return c;
}

// x^(8 n) by the whole wave: lane j holds x^(8 * 2^j) where bit j of n is set, the product goes round in a
// butterfly (six multiplications).  Every lane of the wave must call it; every lane gets the result.
__device__ __forceinline__ uint32_t xpow8_wave(uint64_t n, int lane) {
    uint32_t f = ((n >> (lane & 63)) & 1ull) != 0 ? kCrcTab.pow2[(lane + 3) & 31] : kCrcOne;
    if (lane >= 61) { f = kCrcOne; }
    for (int o = 1; o < 64; o <<= 1) { f = gf_mul(f, (uint32_t)__shfl_xor((int)f, o)); }
    return f;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
    for (int o = 1; o < 64; o <<= 1) { v ^= (uint32_t)__shfl_xor((int)v, o); }
    return v;
}

// bytes [lo, hi) of the 16-byte row at p (16-byte aligned), the others zero: one aligned load for a whole
// row, single bytes otherwise -- nothing outside the range is read
__device__ __forceinline__ uint4 load_row_bytes(const uint8_t* p, uint32_t lo, uint32_t hi) {
    if (lo == 0 && hi >= 16) { return *reinterpret_cast<const uint4*>(p); }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = lo; k < hi && k < 16; k++) { w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3)); }
    uint4 r;
    r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
    return r;
}

// zlib crc32 of a few bytes on one lane (the 28 header bytes of a frame)
__device__ __forceinline__ uint32_t crc32_small(const uint8_t* p, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < n; k++) { c = crc_shift(c ^ p[k], 8); }
    return c ^ 0xFFFFFFFFu;
}

// SQZF version 2 (include/sqz/sqz.h): flags bit 0, bit 31 of an index entry's first word
constexpr uint32_t kFrameStored = 1u;
constexpr uint32_t kFrameDict = 2u;                // version 3: flags bit 1, and the record behind the index
constexpr uint32_t kFrameShuffle = 4u;             // version 4: flags bit 2, and the record behind the index
constexpr uint32_t kStoredBit = 0x80000000u;

// content bytes of block b
__device__ __forceinline__ uint64_t block_len(uint64_t b, uint64_t bb, uint64_t content_bytes) {
    const uint64_t at = b * bb;
    return at >= content_bytes ? 0 : (content_bytes - at < bb ? content_bytes - at : bb);
}
// the writer's rule: a block whose stream is not smaller than its content is stored, padded to 8 bytes
__device__ __forceinline__ bool block_stored(uint64_t stream_bytes, uint64_t len) { return stream_bytes >= len; }
__device__ __forceinline__ uint64_t payload_share(uint64_t stream_bytes, uint64_t len) {
    return block_stored(stream_bytes, len) ? (len + 7) & ~(uint64_t)7 : stream_bytes;
}

__device__ __forceinline__ uint32_t load_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ uint64_t load_le64(const uint8_t* p) {
    return (uint64_t)load_le32(p) | ((uint64_t)load_le32(p + 4) << 32);
}

} // namespace

// crc[b] = zlib.crc32(in[off[b] .. off[b + 1])).  `groups` workgroups share a range (parts of equal size, a
// multiple of 4096, at least kMinPart); with groups > 1 crc[] must be zero at the start: the parts are
// xored in.
__global__ __launch_bounds__(kCrcThreads)
void crc32_blocks_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ off, uint32_t n_ranges,
                         uint32_t* __restrict__ crc, uint32_t groups) {
    __shared__ uint32_t red[2][kCrcThreads / 64];
    const uint32_t b = blockIdx.x / groups, g = blockIdx.x % groups;
    if (b >= n_ranges) { return; }
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t o0 = off[b], o1 = off[b + 1];
    const uint64_t len = o1 > o0 ? o1 - o0 : 0;
    uint64_t part = (len + groups - 1) / groups;
    part = (part + 4095) & ~(uint64_t)4095;
    if (part < kMinPart) { part = kMinPart; }
    const uint64_t s = (uint64_t)g * part < len ? (uint64_t)g * part : len;
    const uint64_t e = len - s > part ? s + part : len;
    if (g != 0 && s >= e) { return; }              // nothing here (the whole workgroup leaves); part 0 stays for the
                                                   // initial value and final xor, also of an empty range
    const uint8_t* const p0 = in + o0 + s;
    const uint64_t plen = e - s;
    const uint32_t head = (uint32_t)((uintptr_t)p0 & 15u);
    const uint8_t* const pa = p0 - head;           // 16-byte aligned; the `head` bytes before p0 count as zeros
    const uint64_t span = plen > 0 ? head + plen : 0;
    const uint64_t nch = (span + kChunk - 1) / kChunk;
    const uint64_t m = nch > 0 ? nch - 1 : 0;      // chunks that end on a chunk boundary; chunk m is the last one
    const uint32_t last_len = (uint32_t)(span - m * kChunk);   // 1..64 (0 for an empty part)

    uint32_t acc = 0, c_last = 0;
    uint64_t jl = 0;
    bool have = false;
    for (uint64_t j = (uint64_t)tid; j < nch; j += kCrcThreads) {
        const uint8_t* const row = pa + j * kChunk;
        const uint32_t lo = j == 0 ? head : 0u;                // first valid byte of the chunk
        const uint32_t hi = j == m ? last_len : kChunk;        // one past its last valid byte
        uint4 r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t a = lo > 16 * k ? lo - 16 * k : 0u;
            const uint32_t z = hi > 16 * k ? hi - 16 * k : 0u;
            if (z > a) { r[k] = load_row_bytes(row + 16 * k, a, z); } else { r[k].x = r[k].y = r[k].z = r[k].w = 0u; }
        }
        const uint32_t w[16] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w,
                                r[2].x, r[2].y, r[2].z, r[2].w, r[3].x, r[3].y, r[3].z, r[3].w};
        uint32_t c = 0;
        if (j < m) {
#pragma unroll
            for (int i = 0; i < 16; i++) { c = crc_word(c ^ w[i]); }
            acc = gf_mul_const<kTileMul>(acc) ^ c;
            jl = j;
            have = true;
        } else {                                   // the last chunk: exactly `hi` bytes (those before `lo` are zeros)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int nb = (int)hi - 4 * i;
                if (nb >= 4) { c = crc_word(c ^ w[i]); }
                else if (nb > 0) { c = crc_shift(c ^ w[i], 8 * nb); }
            }
            c_last = c;
        }
    }
    // every lane's chunks to the end of chunk m - 1, then one value per workgroup
    uint32_t mine = have ? gf_mul(acc, kCrcTab.m512[(m - 1 - jl) & 255u]) : 0u;
    mine = wave_xor(mine);
    c_last = wave_xor(c_last);
    if (lane == 0) { red[0][wave] = mine; red[1][wave] = c_last; }
    __syncthreads();
    if (wave != 0) { return; }
    uint32_t sum = 0, tail = 0;
    for (int k = 0; k < kCrcThreads / 64; k++) { sum ^= red[0][k]; tail ^= red[1][k]; }
    uint32_t r = nch > 0 ? gf_mul(sum, xpow8_wave(last_len, lane)) ^ tail : 0u;
    const uint64_t behind = len - e;               // bytes of the range behind this part
    if (behind > 0) { r = gf_mul(r, xpow8_wave(behind, lane)); }
    if (g == 0) { r ^= gf_mul(0xFFFFFFFFu, xpow8_wave(len, lane)) ^ 0xFFFFFFFFu; }
    if (lane == 0) {
        if (groups == 1) { crc[b] = r; } else { atomicXor(&crc[b], r); }
    }
}

void launch_crc32_blocks(const uint8_t* in, const uint64_t* off, uint32_t n_ranges, uint32_t* crc,
                         uint64_t size_hint, hipStream_t stream) {
    if (n_ranges == 0) { return; }
    // one workgroup per 64 KB of a range when the batch alone does not fill the chip (about 4096 workgroups
    // do); a range whose size the host does not know gets the most, and the surplus leaves at once
    uint64_t groups = size_hint != 0 ? (size_hint + 65535) / 65536 : 1024;
    const uint64_t cap = 4096 / n_ranges > 1 ? 4096 / n_ranges : 1;
    if (groups > cap) { groups = cap; }
    if (groups > 1024) { groups = 1024; }
    if (groups < 1) { groups = 1; }
    while (groups > 1 && groups * n_ranges > 0x7FFFFFFFull) { groups /= 2; }
    if (groups > 1) {
#ifdef SQZ_WAVE_EMU
        memset(crc, 0, (size_t)n_ranges * 4);
#else
        (void)hipMemsetAsync(crc, 0, (size_t)n_ranges * 4, stream);
#endif
    }
    hipLaunchKernelGGL(crc32_blocks_kernel, dim3((unsigned)(groups * n_ranges)), dim3(kCrcThreads), 0, stream,
                       in, off, n_ranges, crc, (uint32_t)groups);
}

// ---------------------------------------------------------------------------------------- encode side
// the uniform cut of a buffer into blocks and of the slab area into slabs, on the device (no host copy)
__global__ __launch_bounds__(256)
void frame_plan_kernel(uint32_t n_blocks, uint64_t block_bytes, uint64_t content_bytes, uint64_t slab_bytes,
                       uint64_t* __restrict__ in_off, uint64_t* __restrict__ slab_off) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_blocks) { return; }
    const uint64_t at = k * block_bytes;
    in_off[k] = at < content_bytes ? at : content_bytes;
    slab_off[k] = k * slab_bytes;
}

void launch_frame_plan(uint32_t n_blocks, uint64_t block_bytes, uint64_t content_bytes, uint64_t slab_bytes,
                       uint64_t* in_off, uint64_t* slab_off, hipStream_t stream) {
    const uint64_t grid = ((uint64_t)n_blocks + 1 + 255) / 256;
    hipLaunchKernelGGL(frame_plan_kernel, dim3((unsigned)grid), dim3(256), 0, stream,
                       n_blocks, block_bytes, content_bytes, slab_bytes, in_off, slab_off);
}

// One workgroup: exclusive scan of the stream sizes, then header, index, padding, the dense offsets for
// compact_blocks_kernel (absolute, from the start of the frame), frame_bytes and the status.  A frame that
// does not fit `capacity`, or a block the encoder failed, leaves the frame untouched: copy_bytes[] = 0 makes
// the compaction a no-op, idx_off = {0, 0} the index checksum an empty range.  The index_crc field is
// written by frame_seal_kernel once the index has been summed.
//
// flags = SQZ_FRAME_STORED writes version 2: block b is stored iff out_bytes[b] >= its length.  A stored block
// takes round_up_8(length) bytes of the payload in the same scan, gets copy_bytes[b] = 0 (the compaction passes
// it by) and stored[b] = 1 (range_copy_kernel moves its content); stored[] is all zeros on a refusal.  With
// flags = 0 stored is not touched and may be null.
//
// kDict (flags has SQZ_FRAME_DICT, with or without SQZ_FRAME_STORED) writes version 3: the record { dict_bytes,
// *dict_crc } directly behind the n entries, payload_off = pad16(32 + 8n + 8) -- the padding now falls on even n --
// and idx_off = {32, 32 + 8n + 8}, so that the index checksum covers the record.  dict_crc is read on the device:
// crc32_blocks_kernel over the dictionary wrote it earlier on the same stream.
//
// kShuf (flags has SQZ_FRAME_SHUFFLE, with or without SQZ_FRAME_STORED; never with kDict) writes version 4: the same
// place and shape, the record being { elem_bytes, 0 } -- elem_bytes comes in dict_bytes' place, dict_crc is not read.
template <bool kDict, bool kShuf = false>
__device__ __forceinline__
void frame_index_body(const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ err,
                      const uint32_t* __restrict__ crc, uint32_t n_blocks, uint64_t content_bytes,
                      uint32_t win_bits, uint32_t block_bits, uint8_t* __restrict__ frame, uint64_t capacity,
                      uint64_t* __restrict__ copy_bytes, uint64_t* __restrict__ dense_off,
                      uint64_t* __restrict__ idx_off, uint64_t* __restrict__ frame_bytes_out,
                      int32_t* __restrict__ status_out, uint32_t flags, uint32_t* __restrict__ stored,
                      uint32_t dict_bytes, const uint32_t* __restrict__ dict_crc) {
    __shared__ uint64_t sums[256];
    __shared__ int32_t first_err[256];
    __shared__ int32_t verdict;
    const uint32_t t = threadIdx.x;
    const uint64_t per = ((uint64_t)n_blocks + 255) / 256;
    const uint64_t b0 = t * per < n_blocks ? t * per : n_blocks;
    const uint64_t b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    const bool store = (flags & kFrameStored) != 0;
    const uint64_t bb = 1ull << block_bits;
    const uint64_t most_words = store || kDict || kShuf ? 0x7FFFFFFFull : 0xFFFFFFFFull;    // bit 31 of the entry is the stored bit
    const uint64_t record = kDict || kShuf ? 8 : 0;
    uint64_t sum = 0;
    int32_t bad = 0;
    for (uint64_t b = b0; b < b1; b++) {
        const uint64_t v = out_bytes[b];
        if (bad == 0 && err[b] != 0) { bad = err[b]; }
        if (bad == 0 && ((v & 7u) != 0 || (v >> 3) > most_words)) { bad = kErrEINVAL; }
        sum += store ? payload_share(v, block_len(b, bb, content_bytes)) : v;
    }
    sums[t] = sum;
    first_err[t] = bad;
    __syncthreads();
    const uint64_t payload_off = (32 + 8 * (uint64_t)n_blocks + record + 15) & ~(uint64_t)15;
    if (t == 0) {
        uint64_t run = 0;
        int32_t st = 0;
        for (int k = 0; k < 256; k++) {
            const uint64_t v = sums[k];
            sums[k] = run;
            run += v;
            if (st == 0) { st = first_err[k]; }
        }
        const uint64_t frame_bytes = payload_off + run;
        if (st == 0 && frame_bytes > capacity) { st = kErrE2BIG; }
        verdict = st;
        *frame_bytes_out = frame_bytes;
        *status_out = st;
        idx_off[0] = st == 0 ? 32 : 0;
        idx_off[1] = st == 0 ? 32 + 8 * (uint64_t)n_blocks + record : 0;
        if (st == 0) {
            uint32_t* const h = reinterpret_cast<uint32_t*>(frame);
            h[0] = 0x465A5153u;                                    // "SQZF"
            h[1] = (kShuf ? 4u : kDict ? 3u : store ? 2u : 1u) | (win_bits << 8) | (block_bits << 16) | ((flags & 0xFFu) << 24);
                                                                   // version, win_bits, block_bits, flags
            h[2] = (uint32_t)content_bytes; h[3] = (uint32_t)(content_bytes >> 32);
            h[4] = (uint32_t)run; h[5] = (uint32_t)(run >> 32);
            h[6] = n_blocks;
            h[7] = 0u;                                             // index_crc: frame_seal_kernel
            uint32_t* const behind = h + 8 + 2 * (uint64_t)n_blocks;       // what follows the n entries
            if (kDict) {
                behind[0] = dict_bytes; behind[1] = *dict_crc;
                if ((n_blocks & 1u) == 0) { behind[2] = 0u; behind[3] = 0u; }
            } else if (kShuf) {
                behind[0] = dict_bytes; behind[1] = 0u;
                if ((n_blocks & 1u) == 0) { behind[2] = 0u; behind[3] = 0u; }
            } else if ((n_blocks & 1u) != 0) { behind[0] = 0u; behind[1] = 0u; }
        }
    }
    __syncthreads();
    const bool ok = verdict == 0;
    uint32_t* const index = reinterpret_cast<uint32_t*>(frame + 32);
    uint64_t at = payload_off + sums[t];
    for (uint64_t b = b0; b < b1; b++) {
        const uint64_t v = out_bytes[b];
        const uint64_t len = block_len(b, bb, content_bytes);
        const bool st = store && block_stored(v, len);
        const uint64_t share = store ? payload_share(v, len) : v;
        dense_off[b] = ok ? at : 0;
        copy_bytes[b] = ok && !st ? v : 0;
        if (store) { stored[b] = ok && st ? 1u : 0u; }
        if (ok) { index[2 * b] = (uint32_t)(share >> 3) | (st ? kStoredBit : 0u); index[2 * b + 1] = crc[b]; }
        at += share;
    }
    if (b1 == n_blocks && (b0 < b1 || t == 0)) { dense_off[n_blocks] = ok ? at : 0; }
}

__global__ __launch_bounds__(256)
void frame_index_kernel(const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ err,
                        const uint32_t* __restrict__ crc, uint32_t n_blocks, uint64_t content_bytes,
                        uint32_t win_bits, uint32_t block_bits, uint8_t* __restrict__ frame, uint64_t capacity,
                        uint64_t* __restrict__ copy_bytes, uint64_t* __restrict__ dense_off,
                        uint64_t* __restrict__ idx_off, uint64_t* __restrict__ frame_bytes_out,
                        int32_t* __restrict__ status_out, uint32_t flags, uint32_t* __restrict__ stored) {
    frame_index_body<false>(out_bytes, err, crc, n_blocks, content_bytes, win_bits, block_bits, frame, capacity,
                            copy_bytes, dense_off, idx_off, frame_bytes_out, status_out, flags, stored, 0u, nullptr);
}

__global__ __launch_bounds__(256)
void frame_index_v3_kernel(const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ err,
                           const uint32_t* __restrict__ crc, uint32_t n_blocks, uint64_t content_bytes,
                           uint32_t win_bits, uint32_t block_bits, uint8_t* __restrict__ frame, uint64_t capacity,
                           uint64_t* __restrict__ copy_bytes, uint64_t* __restrict__ dense_off,
                           uint64_t* __restrict__ idx_off, uint64_t* __restrict__ frame_bytes_out,
                           int32_t* __restrict__ status_out, uint32_t flags, uint32_t* __restrict__ stored,
                           uint32_t dict_bytes, const uint32_t* __restrict__ dict_crc) {
    frame_index_body<true>(out_bytes, err, crc, n_blocks, content_bytes, win_bits, block_bits, frame, capacity,
                           copy_bytes, dense_off, idx_off, frame_bytes_out, status_out, flags, stored, dict_bytes,
                           dict_crc);
}

__global__ __launch_bounds__(256)
void frame_index_v4_kernel(const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ err,
                           const uint32_t* __restrict__ crc, uint32_t n_blocks, uint64_t content_bytes,
                           uint32_t win_bits, uint32_t block_bits, uint8_t* __restrict__ frame, uint64_t capacity,
                           uint64_t* __restrict__ copy_bytes, uint64_t* __restrict__ dense_off,
                           uint64_t* __restrict__ idx_off, uint64_t* __restrict__ frame_bytes_out,
                           int32_t* __restrict__ status_out, uint32_t flags, uint32_t* __restrict__ stored,
                           uint32_t elem_bytes) {
    frame_index_body<false, true>(out_bytes, err, crc, n_blocks, content_bytes, win_bits, block_bits, frame, capacity,
                                  copy_bytes, dense_off, idx_off, frame_bytes_out, status_out, flags, stored,
                                  elem_bytes, nullptr);
}

void launch_frame_index(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                        uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint8_t* frame,
                        uint64_t capacity, uint64_t* copy_bytes, uint64_t* dense_off, uint64_t* idx_off,
                        uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frame_index_kernel, dim3(1), dim3(256), 0, stream, out_bytes, err, crc, n_blocks,
                       content_bytes, win_bits, block_bits, frame, capacity, copy_bytes, dense_off, idx_off,
                       frame_bytes_out, status_out, 0u, (uint32_t*)nullptr);
}

void launch_frame_index_v2(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                           uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint8_t* frame,
                           uint64_t capacity, uint64_t* copy_bytes, uint64_t* dense_off, uint32_t* stored,
                           uint64_t* idx_off, uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frame_index_kernel, dim3(1), dim3(256), 0, stream, out_bytes, err, crc, n_blocks,
                       content_bytes, win_bits, block_bits, frame, capacity, copy_bytes, dense_off, idx_off,
                       frame_bytes_out, status_out, kFrameStored, stored);
}

void launch_frame_index_v3(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                           uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                           uint32_t dict_bytes, const uint32_t* dict_crc, uint8_t* frame, uint64_t capacity,
                           uint64_t* copy_bytes, uint64_t* dense_off, uint32_t* stored, uint64_t* idx_off,
                           uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frame_index_v3_kernel, dim3(1), dim3(256), 0, stream, out_bytes, err, crc, n_blocks,
                       content_bytes, win_bits, block_bits, frame, capacity, copy_bytes, dense_off, idx_off,
                       frame_bytes_out, status_out, (flags & kFrameStored) | kFrameDict, stored, dict_bytes, dict_crc);
}

void launch_frame_index_v4(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc, uint32_t n_blocks,
                           uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                           uint32_t elem_bytes, uint8_t* frame, uint64_t capacity, uint64_t* copy_bytes,
                           uint64_t* dense_off, uint32_t* stored, uint64_t* idx_off, uint64_t* frame_bytes_out,
                           int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frame_index_v4_kernel, dim3(1), dim3(256), 0, stream, out_bytes, err, crc, n_blocks,
                       content_bytes, win_bits, block_bits, frame, capacity, copy_bytes, dense_off, idx_off,
                       frame_bytes_out, status_out, (flags & kFrameStored) | kFrameShuffle, stored, elem_bytes);
}

// index_crc = crc32(header[0, 28) || index): the header's 28 bytes on the spot, joined with the index's
// checksum (idx_crc, from crc32_blocks_kernel) by crc(A || B) = crc(A) * x^(8|B|) ^ crc(B).  idx_bytes: what
// idx_crc covers, 8 n_blocks, and 8 more in a version-3 frame (the dictionary's record)
__global__ __launch_bounds__(64)
void frame_seal_kernel(uint8_t* __restrict__ frame, const uint32_t* __restrict__ idx_crc, uint64_t idx_bytes,
                       const int32_t* __restrict__ status) {
    const int lane = (int)threadIdx.x;
    if (*status != 0) { return; }
    const uint32_t h = crc32_small(frame, 28);
    const uint32_t c = gf_mul(h, xpow8_wave(idx_bytes, lane)) ^ *idx_crc;
    if (lane == 0) { reinterpret_cast<uint32_t*>(frame)[7] = c; }
}

void launch_frame_seal(uint8_t* frame, const uint32_t* idx_crc, uint32_t n_blocks, const int32_t* status,
                       hipStream_t stream, uint32_t record_bytes) {
    hipLaunchKernelGGL(frame_seal_kernel, dim3(1), dim3(64), 0, stream, frame, idx_crc,
                       8 * (uint64_t)n_blocks + record_bytes, status);
}

// ---------------------------------------------------------------------------------------- decode side
// One workgroup.  The caller read n_blocks and content_bytes from a host copy of the header and made sure
// that avail covers header and index; idx_crc is the checksum of frame[32, 32 + 8 n) computed just before.
// Checks that the device header says the same, every field's range, index_crc, the sum of stream_words
// and that the payload lies inside avail.  Then in_off (absolute, from the start of the frame) and out_off
// (from the start of block `first`) for blocks [first, first + n_sel).  On any failure *status is set and
// every selected block gets a zero-length input and output: nothing behind the index is ever addressed.
//
// A version-2 frame (flags = SQZ_FRAME_STORED) needs `stored` (n_sel entries; EINVAL without it): bit 31 of an
// entry's first word marks a stored block, the other 31 bits are its share of the payload in words, which for a
// stored block must be ceil(length / 8) exactly (EINVAL, checked once index_crc has held).  stored[k] = 1 for a
// selected stored block, 0 otherwise -- all zeros for a version-1 frame and on any refusal.
//
// kDict is the reader of version 3, and of nothing else (versions 1 and 2 are EINVAL through it, as version 3 is
// through the other).  idx_crc then covers frame[32, 32 + 8 n + 8), the index and the record; dict_bytes and
// *dict_crc describe the dictionary the caller brought (crc32_blocks_kernel over it, earlier on the stream).  The
// checks in the host's order (sqz_frame_info, then its dictionary check): header fields EINVAL, header against the
// arguments EINVAL, index_crc EILSEQ, the record's dict_bytes outside 1 .. window - 1 EINVAL, a stored entry without
// flags bit 0 or of the wrong size EINVAL, the words' sum EINVAL, a record that is not (dict_bytes, *dict_crc)
// EILSEQ, the payload beyond avail E2BIG.
// want_bits (either flavour): the block_bits the caller's own arithmetic used, 0 when it used none; a frame with
// another is EINVAL with the header's other disagreements (a ranged read works first and n_sel out on the host).
//
// kList is the open of a gather (many ranges in one call): the same checks in the same order (first = n_sel = 0),
// and offsets for the blocks whose bit is set in `bitmap` instead of a run of them.  gather_select_kernel has left
// wpre (set bits in front of every bitmap word: block b's slot is wpre[b / 32] + popc of the bits below b), sel (the
// blocks in ascending order), ctl[0] (how many) and ctl[1] (ENOBUFS / ENOSPC / 0).  The decode kernels take a
// stream as in[in_off[j], in_off[j + 1]), which a selection with gaps cannot give directly, so a slot k has TWO
// entries: 2k is the block sel[k], 2k + 1 a pseudo-block that covers the bytes up to the next selected stream and
// is switched off through skip[].  Slot k decodes to [k * block_bytes, ..): a range's covering blocks are
// consecutive slots, so it lies in one piece.  *status_out = the frame's status, else ctl[1]; *blocks_decoded = 0
// for a refused frame, else ctl[0].  With any status every one of the 2 * max_blocks entries is empty and skipped,
// as are the entries behind slot ctl[0] otherwise: the launch behind this one is sized for max_blocks on the host.
//
// kShuf is the reader of version 4, and of nothing else (never with kDict or kList).  idx_crc covers index and record
// as for version 3; dict_bytes is the elem_bytes the caller read from its copy of the record, dict_crc is not read.
// Its checks in the host's order: as above up to index_crc, then a record that is not { 2 | 4 | 8, 0 } or whose
// elem_bytes is not the caller's EINVAL, then the stored entries and what follows them.
template <bool kDict, bool kList = false, bool kShuf = false>
__device__ __forceinline__
void frame_open_body(const uint8_t* __restrict__ frame, uint64_t avail, uint32_t n_blocks,
                     uint64_t content_bytes, uint32_t first, uint32_t n_sel,
                     const uint32_t* __restrict__ idx_crc, uint64_t* __restrict__ in_off,
                     uint64_t* __restrict__ out_off, int32_t* __restrict__ status_out,
                     uint32_t* __restrict__ stored, uint32_t dict_bytes, const uint32_t* __restrict__ dict_crc,
                     uint32_t want_bits, const uint32_t* __restrict__ bitmap = nullptr,
                     const uint32_t* __restrict__ wpre = nullptr, const uint32_t* __restrict__ sel = nullptr,
                     const uint32_t* __restrict__ ctl = nullptr, uint32_t max_blocks = 0,
                     uint32_t* __restrict__ skip = nullptr, uint32_t* __restrict__ blocks_decoded = nullptr) {
    __shared__ uint64_t sums[256];
    __shared__ uint32_t wrong[256];
    __shared__ int32_t verdict;
    __shared__ uint32_t want_crc;
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u);
    if (t < 64) {                                  // wave 0, all of it: what index_crc has to be
        const uint32_t h = crc32_small(frame, 28);
        const uint32_t c = gf_mul(h, xpow8_wave(8 * (uint64_t)n_blocks + (kDict || kShuf ? 8 : 0), lane)) ^ *idx_crc;
        if (lane == 0) { want_crc = c; }
    }
    const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
    const uint64_t per = ((uint64_t)n_blocks + 255) / 256;
    const uint64_t b0 = t * per < n_blocks ? t * per : n_blocks;
    const uint64_t b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    const uint32_t block_bits = frame[6];
    const bool v2 = kShuf ? frame[4] == 4 : kDict ? frame[4] == 3 : frame[4] == 2;         // an entry's bit 31 is the stored bit
    const bool may_store = !(kDict || kShuf) || (frame[7] & kFrameStored) != 0;    // versions 3 and 4 have the bit with or without the flag
    const uint32_t words_mask = v2 ? ~kStoredBit : 0xFFFFFFFFu;
    uint64_t sum = 0;
    uint32_t misfit = 0;                           // a stored entry whose size is not its block's, or in a frame without any
    for (uint64_t b = b0; b < b1; b++) {
        const uint32_t e = index[2 * b];
        if (v2 && (e & kStoredBit) != 0 && block_bits <= 24 &&
            (!may_store ||
             (uint64_t)(e & words_mask) != (block_len(b, 1ull << block_bits, content_bytes) + 7) / 8)) { misfit = 1; }
        sum += (uint64_t)(e & words_mask) * 8;
    }
    sums[t] = sum;
    wrong[t] = misfit;
    __syncthreads();
    const uint64_t payload_off = (32 + 8 * (uint64_t)n_blocks + (kDict || kShuf ? 8 : 0) + 15) & ~(uint64_t)15;
    if (t == 0) {
        uint64_t run = 0;
        bool beyond = false;                       // the streams add up to more than there is: stop adding (no wrap)
        uint32_t any_misfit = 0;
        for (int k = 0; k < 256; k++) {
            const uint64_t v = sums[k];            // < 2^59: at most 2^24 entries of less than 2^35 each
            sums[k] = run;
            if (v > avail || run > avail - v) { beyond = true; } else { run += v; }
            any_misfit |= wrong[k];
        }
        int32_t st = 0;
        const uint32_t win_bits = frame[5];
        // version 1 has no flags; version 2 has some, all of them known, and needs somewhere to put the mask;
        // version 3 has bit 1, perhaps bit 0, no other, and needs the mask as well
        const bool version_ok = kShuf ? frame[4] == 4 && (frame[7] & kFrameShuffle) != 0 &&
                                        (frame[7] & ~(kFrameStored | kFrameShuffle)) == 0 && (stored != nullptr || n_sel == 0)
                              : kDict ? frame[4] == 3 && (frame[7] & kFrameDict) != 0 &&
                                        (frame[7] & ~(kFrameStored | kFrameDict)) == 0 && (stored != nullptr || n_sel == 0)
                                      : (frame[4] == 1 && frame[7] == 0) ||
                                        (frame[4] == 2 && frame[7] == kFrameStored && (stored != nullptr || n_sel == 0));
        const uint8_t* const rec = frame + 32 + 8 * (uint64_t)n_blocks;    // (version 3: the caller saw to avail)
        if (load_le32(frame) != 0x465A5153u || !version_ok || win_bits < 10 || win_bits > 15 ||
            block_bits < 12 || block_bits > 24) {
            st = kErrEINVAL;
        } else {
            const uint64_t bb = 1ull << block_bits;
            const uint64_t want_n = content_bytes / bb + ((content_bytes & (bb - 1)) != 0 ? 1 : 0);
            if (load_le64(frame + 8) != content_bytes || load_le32(frame + 24) != n_blocks || want_n != n_blocks ||
                (uint64_t)first + n_sel > n_blocks || (want_bits != 0 && block_bits != want_bits)) {
                st = kErrEINVAL;
            } else if (load_le32(frame + 28) != want_crc) {
                st = kErrEILSEQ;
            } else if (kDict && (load_le32(rec) == 0 || load_le32(rec) > (1u << win_bits) - 1u)) {
                st = kErrEINVAL;
            } else if (kShuf && ((load_le32(rec) != 2u && load_le32(rec) != 4u && load_le32(rec) != 8u) ||
                                 load_le32(rec + 4) != 0u || load_le32(rec) != dict_bytes)) {
                st = kErrEINVAL;
            } else if (any_misfit != 0) {
                st = kErrEINVAL;
            } else if (!beyond && load_le64(frame + 16) != run) {
                st = kErrEINVAL;
            } else if (kDict && (load_le32(rec) != dict_bytes || load_le32(rec + 4) != *dict_crc)) {
                st = kErrEILSEQ;
            } else if (beyond || payload_off > avail || run > avail - payload_off) {
                st = kErrE2BIG;
            }
        }
        if constexpr (kList) {                     // a frame that holds: the verdict on the two caps
            *blocks_decoded = st != 0 ? 0u : ctl[0];
            if (st == 0) { st = (int32_t)ctl[1]; }
        }
        verdict = st;
        *status_out = st;
    }
    __syncthreads();
    if constexpr (kList) {
        const uint64_t entries = 2 * (uint64_t)max_blocks;
        if (verdict != 0) {                        // refused, or a cap too small: nothing is decoded
            for (uint64_t k = t; k <= entries; k += 256) {
                in_off[k] = 0; out_off[k] = 0;
                if (k < entries) { stored[k] = 0; skip[k] = 1; }
            }
            return;
        }
        const uint64_t bb = 1ull << block_bits;
        const uint32_t count = ctl[0];             // <= max_blocks: ctl[1] == 0
        uint64_t at = payload_off + sums[t];
        for (uint64_t b = b0; b < b1; b++) {
            const uint32_t e = index[2 * b];
            const uint64_t share = (uint64_t)(e & words_mask) * 8;
            const uint32_t w = bitmap[b >> 5], bit = (uint32_t)b & 31u;
            if (((w >> bit) & 1u) != 0) {
                const uint64_t k = wpre[b >> 5] + (uint32_t)__builtin_popcount(w & ((1u << bit) - 1u));
                if (k < count) {
                    const uint32_t raw = v2 && (e & kStoredBit) != 0 ? 1u : 0u;
                    in_off[2 * k] = at; in_off[2 * k + 1] = at + share;
                    out_off[2 * k] = k * bb; out_off[2 * k + 1] = k * bb + block_len(b, bb, content_bytes);
                    stored[2 * k] = raw; stored[2 * k + 1] = 0;
                    skip[2 * k] = raw; skip[2 * k + 1] = 1;
                }
            }
            at += share;
        }
        // behind the last slot in use: empty entries at the end of the payload (payload_bytes is the sum: checked)
        // and at the end of the decoded bytes; entry 2 count - 1 reaches up to them
        const uint64_t end_in = payload_off + load_le64(frame + 16);
        const uint64_t end_out = count == 0 ? 0 : (uint64_t)(count - 1) * bb + block_len(sel[count - 1], bb, content_bytes);
        for (uint64_t k = 2 * (uint64_t)count + t; k <= entries; k += 256) {
            in_off[k] = end_in; out_off[k] = end_out;
            if (k < entries) { stored[k] = 0; skip[k] = 1; }
        }
        return;
    }
    if (verdict != 0) {                            // refused: nothing below looks at the index again
        for (uint64_t k = t; k <= n_sel; k += 256) {
            in_off[k] = 0; out_off[k] = 0;
            if (stored != nullptr && k < n_sel) { stored[k] = 0; }
        }
        return;
    }
    const uint64_t bb = 1ull << block_bits;
    const uint64_t base = (uint64_t)first * bb;
    uint64_t at = payload_off + sums[t];
    for (uint64_t b = b0; b < b1; b++) {
        const uint32_t e = index[2 * b];
        if (b >= first && b <= (uint64_t)first + n_sel) { in_off[b - first] = at; }
        if (stored != nullptr && b >= first && b < (uint64_t)first + n_sel) {
            stored[b - first] = v2 && (e & kStoredBit) != 0 ? 1u : 0u;
        }
        at += (uint64_t)(e & words_mask) * 8;
    }
    if (b1 == n_blocks && (b0 < b1 || t == 0) && (uint64_t)first + n_sel == n_blocks) { in_off[n_sel] = at; }
    for (uint64_t k = t; k <= n_sel; k += 256) {
        const uint64_t o = (first + k) * bb < content_bytes ? (first + k) * bb : content_bytes;
        out_off[k] = o - base;
    }
}

__global__ __launch_bounds__(256)
void frame_open_kernel(const uint8_t* __restrict__ frame, uint64_t avail, uint32_t n_blocks,
                       uint64_t content_bytes, uint32_t first, uint32_t n_sel,
                       const uint32_t* __restrict__ idx_crc, uint64_t* __restrict__ in_off,
                       uint64_t* __restrict__ out_off, int32_t* __restrict__ status_out,
                       uint32_t* __restrict__ stored, uint32_t want_bits) {
    frame_open_body<false>(frame, avail, n_blocks, content_bytes, first, n_sel, idx_crc, in_off, out_off, status_out,
                           stored, 0u, nullptr, want_bits);
}

__global__ __launch_bounds__(256)
void frame_open_v3_kernel(const uint8_t* __restrict__ frame, uint64_t avail, uint32_t n_blocks,
                          uint64_t content_bytes, uint32_t first, uint32_t n_sel,
                          const uint32_t* __restrict__ idx_crc, uint64_t* __restrict__ in_off,
                          uint64_t* __restrict__ out_off, int32_t* __restrict__ status_out,
                          uint32_t* __restrict__ stored, uint32_t dict_bytes, const uint32_t* __restrict__ dict_crc,
                          uint32_t want_bits) {
    frame_open_body<true>(frame, avail, n_blocks, content_bytes, first, n_sel, idx_crc, in_off, out_off, status_out,
                          stored, dict_bytes, dict_crc, want_bits);
}

__global__ __launch_bounds__(256)
void frame_open_v4_kernel(const uint8_t* __restrict__ frame, uint64_t avail, uint32_t n_blocks,
                          uint64_t content_bytes, uint32_t first, uint32_t n_sel,
                          const uint32_t* __restrict__ idx_crc, uint64_t* __restrict__ in_off,
                          uint64_t* __restrict__ out_off, int32_t* __restrict__ status_out,
                          uint32_t* __restrict__ stored, uint32_t elem_bytes, uint32_t want_bits) {
    frame_open_body<false, false, true>(frame, avail, n_blocks, content_bytes, first, n_sel, idx_crc, in_off, out_off,
                                        status_out, stored, elem_bytes, nullptr, want_bits);
}

void launch_frame_open(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                       uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint64_t* in_off,
                       uint64_t* out_off, int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frame_open_kernel, dim3(1), dim3(256), 0, stream, frame, avail, n_blocks, content_bytes,
                       first, n_sel, idx_crc, in_off, out_off, status_out, (uint32_t*)nullptr, 0u);
}

void launch_frame_open_v2(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                          uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint64_t* in_off,
                          uint64_t* out_off, uint32_t* stored, int32_t* status_out, hipStream_t stream,
                          uint32_t want_bits) {
    hipLaunchKernelGGL(frame_open_kernel, dim3(1), dim3(256), 0, stream, frame, avail, n_blocks, content_bytes,
                       first, n_sel, idx_crc, in_off, out_off, status_out, stored, want_bits);
}

void launch_frame_open_v3(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                          uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint32_t dict_bytes,
                          const uint32_t* dict_crc, uint64_t* in_off, uint64_t* out_off, uint32_t* stored,
                          int32_t* status_out, hipStream_t stream, uint32_t want_bits) {
    hipLaunchKernelGGL(frame_open_v3_kernel, dim3(1), dim3(256), 0, stream, frame, avail, n_blocks, content_bytes,
                       first, n_sel, idx_crc, in_off, out_off, status_out, stored, dict_bytes, dict_crc, want_bits);
}

void launch_frame_open_v4(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                          uint32_t first, uint32_t n_sel, const uint32_t* idx_crc, uint32_t elem_bytes,
                          uint64_t* in_off, uint64_t* out_off, uint32_t* stored, int32_t* status_out,
                          hipStream_t stream, uint32_t want_bits) {
    hipLaunchKernelGGL(frame_open_v4_kernel, dim3(1), dim3(256), 0, stream, frame, avail, n_blocks, content_bytes,
                       first, n_sel, idx_crc, in_off, out_off, status_out, stored, elem_bytes, want_bits);
}

__global__ __launch_bounds__(256)
void frame_open_list_kernel(const uint8_t* __restrict__ frame, uint64_t avail, uint32_t n_blocks,
                            uint64_t content_bytes, const uint32_t* __restrict__ idx_crc,
                            const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                            const uint32_t* __restrict__ sel, const uint32_t* __restrict__ ctl, uint32_t max_blocks,
                            uint64_t* __restrict__ in_off, uint64_t* __restrict__ out_off,
                            uint32_t* __restrict__ skip, uint32_t* __restrict__ stored,
                            int32_t* __restrict__ status_out, uint32_t* __restrict__ blocks_decoded,
                            uint32_t want_bits) {
    frame_open_body<false, true>(frame, avail, n_blocks, content_bytes, 0u, 0u, idx_crc, in_off, out_off, status_out,
                                 stored, 0u, nullptr, want_bits, bitmap, wpre, sel, ctl, max_blocks, skip,
                                 blocks_decoded);
}

__global__ __launch_bounds__(256)
void frame_open_list_v3_kernel(const uint8_t* __restrict__ frame, uint64_t avail, uint32_t n_blocks,
                               uint64_t content_bytes, const uint32_t* __restrict__ idx_crc,
                               const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                               const uint32_t* __restrict__ sel, const uint32_t* __restrict__ ctl, uint32_t max_blocks,
                               uint64_t* __restrict__ in_off, uint64_t* __restrict__ out_off,
                               uint32_t* __restrict__ skip, uint32_t* __restrict__ stored,
                               int32_t* __restrict__ status_out, uint32_t* __restrict__ blocks_decoded,
                               uint32_t dict_bytes, const uint32_t* __restrict__ dict_crc, uint32_t want_bits) {
    frame_open_body<true, true>(frame, avail, n_blocks, content_bytes, 0u, 0u, idx_crc, in_off, out_off, status_out,
                                stored, dict_bytes, dict_crc, want_bits, bitmap, wpre, sel, ctl, max_blocks, skip,
                                blocks_decoded);
}

void launch_frame_open_list(const uint8_t* frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                            const uint32_t* idx_crc, uint32_t dict_bytes, const uint32_t* dict_crc,
                            const uint32_t* bitmap, const uint32_t* wpre, const uint32_t* sel, const uint32_t* ctl,
                            uint32_t max_blocks, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                            int32_t* status_out, uint32_t* blocks_decoded, hipStream_t stream, uint32_t want_bits) {
    if (dict_crc != nullptr) {
        hipLaunchKernelGGL(frame_open_list_v3_kernel, dim3(1), dim3(256), 0, stream, frame, avail, n_blocks,
                           content_bytes, idx_crc, bitmap, wpre, sel, ctl, max_blocks, in_off, out_off, skip, stored,
                           status_out, blocks_decoded, dict_bytes, dict_crc, want_bits);
    } else {
        hipLaunchKernelGGL(frame_open_list_kernel, dim3(1), dim3(256), 0, stream, frame, avail, n_blocks,
                           content_bytes, idx_crc, bitmap, wpre, sel, ctl, max_blocks, in_off, out_off, skip, stored,
                           status_out, blocks_decoded, want_bits);
    }
}

// err[k] for the selected blocks: the frame's status where it was refused; EILSEQ where the decoder was
// content but the bytes are not the ones that were checksummed; else what the decoder said
__global__ __launch_bounds__(256)
void frame_verify_kernel(const uint8_t* __restrict__ frame, uint32_t first, uint32_t n_sel,
                         const uint32_t* __restrict__ crc, const int32_t* __restrict__ status,
                         int32_t* __restrict__ err) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_sel) { return; }
    const int32_t st = *status;
    if (st != 0) { err[k] = st; return; }
    const uint32_t stored = reinterpret_cast<const uint32_t*>(frame + 32)[2 * ((uint64_t)first + k) + 1];
    if (err[k] == 0 && crc[k] != stored) { err[k] = kErrEILSEQ; }
}

void launch_frame_verify(const uint8_t* frame, uint32_t first, uint32_t n_sel, const uint32_t* crc,
                         const int32_t* status, int32_t* err, hipStream_t stream) {
    if (n_sel == 0) { return; }
    hipLaunchKernelGGL(frame_verify_kernel, dim3((n_sel + 255) / 256), dim3(256), 0, stream,
                       frame, first, n_sel, crc, status, err);
}

// A ranged read from a resident frame, once the covering blocks [first, first + n_sel) lie decoded and verified in
// scratch: *status = the frame's status, otherwise the first non-zero err[k]; and a one-range work list for
// range_copy_kernel -- `length` bytes from `src_at` (the range's place in the decoded blocks) to the start of the
// caller's buffer, masked out unless everything held, so that the copy moves the range or nothing.
// plan: src_off = plan[0], dst_off = len_off = plan + 2 ({0, length}), mask = (uint32_t*)(plan + 4).
__global__ __launch_bounds__(256)
void frame_read_plan_kernel(const int32_t* __restrict__ err, uint32_t n_sel, uint64_t src_at, uint64_t length,
                            uint64_t* __restrict__ plan, int32_t* __restrict__ status) {
    __shared__ uint32_t first_bad[256];
    const uint32_t t = threadIdx.x;
    uint32_t mine = 0xFFFFFFFFu;                   // the first block of this lane's that failed
    for (uint64_t k = t; k < n_sel; k += 256) {
        if (err[k] != 0) { mine = (uint32_t)k; break; }
    }
    first_bad[t] = mine;
    __syncthreads();
    if (t != 0) { return; }
    uint32_t bad = 0xFFFFFFFFu;
    for (int k = 0; k < 256; k++) { bad = first_bad[k] < bad ? first_bad[k] : bad; }
    int32_t st = *status;
    if (st == 0 && bad != 0xFFFFFFFFu) { st = err[bad]; }
    *status = st;
    plan[0] = src_at;
    plan[2] = 0; plan[3] = length;
    *reinterpret_cast<uint32_t*>(plan + 4) = st == 0 ? 1u : 0u;
}

void launch_frame_read_plan(const int32_t* err, uint32_t n_sel, uint64_t src_at, uint64_t length, uint64_t* plan,
                            int32_t* status, hipStream_t stream) {
    hipLaunchKernelGGL(frame_read_plan_kernel, dim3(1), dim3(256), 0, stream, err, n_sel, src_at, length, plan, status);
}

// ---------------------------------------------------------------------------------------- stored blocks
// Ragged range copy: range b is len_off[b + 1] - len_off[b] bytes from src + src_off[b] to dst + dst_off[b], for
// the ranges whose mask[b] is non-zero (all of them with a null mask); with pad8 the destination is filled with
// zeros up to the next multiple of 8 bytes of its length.  len_off is src_off (encode: content into the payload)
// or dst_off (decode: payload into the output).  Nothing is assumed about alignment and nothing outside a range
// is read or, padding aside, written: the destination is cut into 16-byte rows on ADDRESS boundaries, every full
// row is one aligned 16-byte store, and its source bytes are one aligned 16-byte load when both sides share the
// alignment, two aligned loads joined by a byte shift when they do not and both source rows lie inside the
// range, single bytes otherwise (the first and last rows of a misaligned range).  `groups` workgroups share a
// range row by row, so one 16 MB block fills the chip as 4096 blocks of 256 KB do.
constexpr int kCopyThreads = 256;

__device__ __forceinline__ uint64_t join_bytes(uint64_t lo, uint64_t hi, uint32_t s) {     // bytes s .. s + 7 of lo:hi
    return s == 0 ? lo : (lo >> (8 * s)) | (hi << (64 - 8 * s));
}

__global__ __launch_bounds__(kCopyThreads)
void range_copy_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off,
                       uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_off,
                       const uint64_t* __restrict__ len_off, const uint32_t* __restrict__ mask, uint32_t n_ranges,
                       uint32_t pad8, uint32_t groups) {
    const uint32_t b = blockIdx.x / groups, g = blockIdx.x % groups;
    if (b >= n_ranges) { return; }
    if (mask != nullptr && mask[b] == 0) { return; }
    const uint64_t l0 = len_off[b], l1 = len_off[b + 1];
    const uint64_t len = l1 > l0 ? l1 - l0 : 0;
    const uint8_t* const from = src + src_off[b];
    uint8_t* const to = dst + dst_off[b];
    const uint32_t tid = threadIdx.x;
    uint64_t head = (16u - (uint32_t)((uintptr_t)to & 15u)) & 15u;     // bytes in front of the first full row
    if (head > len) { head = len; }
    const uint64_t rows = (len - head) / 16;
    const uint64_t tail_at = head + 16 * rows;                         // bytes behind the last full row
    if (g == 0) {
        if (tid < head) { to[tid] = from[tid]; }
        if (tid >= 32 && tid - 32 < len - tail_at) { to[tail_at + (tid - 32)] = from[tail_at + (tid - 32)]; }
        const uint64_t padded = (len + 7) & ~(uint64_t)7;
        if (pad8 != 0 && tid >= 64 && len + (tid - 64) < padded) { to[len + (tid - 64)] = 0; }
    }
    const uint8_t* const fb = from + head;
    uint8_t* const tb = to + head;                                     // 16-byte aligned
    const uint32_t sh = (uint32_t)((uintptr_t)fb & 15u);               // where a row's bytes start in their source row
    const uint8_t* const src_end = from + len;
    for (uint64_t k = (uint64_t)g * kCopyThreads + tid; k < rows; k += (uint64_t)groups * kCopyThreads) {
        const uint8_t* const sp = fb + 16 * k;
        uint4 v;
        if (sh == 0) {
            v = *reinterpret_cast<const uint4*>(sp);
        } else if (sp - sh >= from && sp - sh + 32 <= src_end) {
            const uint4 a = *reinterpret_cast<const uint4*>(sp - sh);
            const uint4 c = *reinterpret_cast<const uint4*>(sp - sh + 16);
            const uint64_t q0 = (uint64_t)a.x | ((uint64_t)a.y << 32), q1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
            const uint64_t q2 = (uint64_t)c.x | ((uint64_t)c.y << 32), q3 = (uint64_t)c.z | ((uint64_t)c.w << 32);
            const bool up = sh >= 8;
            const uint32_t s = sh & 7u;
            const uint64_t lo = join_bytes(up ? q1 : q0, up ? q2 : q1, s);
            const uint64_t hi = join_bytes(up ? q2 : q1, up ? q3 : q2, s);
            v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
        } else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};       // a source row that is not whole inside the range: byte by byte
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) { w[j >> 2] |= (uint32_t)sp[j] << (8 * (j & 3)); }
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *reinterpret_cast<uint4*>(tb + 16 * k) = v;
    }
}

void launch_range_copy(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                       const uint64_t* len_off, const uint32_t* mask, uint32_t n_ranges, bool pad8,
                       uint64_t size_hint, hipStream_t stream) {
    if (n_ranges == 0) { return; }
    // one workgroup per 32 KB of a range, about 8192 workgroups at the most; the workgroups of a range that is
    // left out, or is shorter than the hint, leave at once
    uint64_t groups = size_hint != 0 ? (size_hint + 32767) / 32768 : 512;
    const uint64_t cap = 8192 / n_ranges > 1 ? 8192 / n_ranges : 1;
    if (groups > cap) { groups = cap; }
    if (groups > 2048) { groups = 2048; }
    if (groups < 1) { groups = 1; }
    while (groups > 1 && groups * n_ranges > 0x7FFFFFFFull) { groups /= 2; }
    hipLaunchKernelGGL(range_copy_kernel, dim3((unsigned)(groups * n_ranges)), dim3(kCopyThreads), 0, stream,
                       src, src_off, dst, dst_off, len_off, mask, n_ranges, pad8 ? 1u : 0u, (uint32_t)groups);
}

// ---------------------------------------------------------------------------------------- gather
// Many byte ranges of a resident frame in one call ("Gather").  offset[] and length[] lie in
// device memory; the host knows their number, max_length (a cap on every length) and max_blocks (a cap on the
// distinct covering blocks).  mark -> select -> open for a list (frame_open_body<.., true>) -> the decode chain ->
// plan -> copy.
constexpr int kErrENOBUFS = 105, kErrENOSPC = 28;  // <errno.h>, checked in abi.hip
constexpr int kGatherThreads = 256;

// a range the call delivers: no longer than the cap, inside the content, offset + length without a wrap
__device__ __forceinline__ bool gather_range_ok(uint64_t off, uint64_t len, uint64_t max_length,
                                                uint64_t content_bytes) {
    return len <= max_length && off <= content_bytes && len <= content_bytes - off;
}

// One lane per range: the bits of its covering blocks into bitmap (n_blocks bits, zero at the start), a word at a
// time.  max_length bounds the loop: ((max_length + 2^b - 2) >> b) + 1 blocks at the most, 32 to a word.
__global__ __launch_bounds__(kGatherThreads)
void gather_mark_kernel(const uint64_t* __restrict__ offset, const uint64_t* __restrict__ length, uint32_t n_ranges,
                        uint64_t max_length, uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks,
                        uint32_t* __restrict__ bitmap) {
    const uint64_t r = (uint64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    if (r >= n_ranges) { return; }
    const uint64_t off = offset[r], len = length[r];
    if (len == 0 || !gather_range_ok(off, len, max_length, content_bytes)) { return; }
    const uint64_t first = off >> block_bits;
    uint64_t last = (off + len - 1) >> block_bits;
    if (first >= n_blocks) { return; }             // (n_blocks is ceil(content / 2^b), the call checked: never taken)
    if (last >= n_blocks) { last = (uint64_t)n_blocks - 1; }
    for (uint64_t w = first >> 5; w <= last >> 5; w++) {
        const uint32_t lo = w == first >> 5 ? (uint32_t)first & 31u : 0u;
        const uint32_t hi = w == last >> 5 ? (uint32_t)last & 31u : 31u;
        const uint32_t bits = (0xFFFFFFFFu >> (31u - hi)) & (0xFFFFFFFFu << lo);
#ifdef SQZ_WAVE_EMU
        bitmap[w] |= bits;                         // lanes run one after the other there: a plain read-modify-write
#else
        atomicOr(&bitmap[w], bits);
#endif
    }
}

void launch_gather_mark(const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                        uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks, uint32_t* bitmap,
                        hipStream_t stream) {
    const uint64_t words = ((uint64_t)n_blocks + 31) / 32;
#ifdef SQZ_WAVE_EMU
    memset(bitmap, 0, (size_t)words * 4);
#else
    if (words > 0) { (void)hipMemsetAsync(bitmap, 0, (size_t)words * 4, stream); }
#endif
    if (n_ranges == 0) { return; }
    const uint64_t grid = ((uint64_t)n_ranges + kGatherThreads - 1) / kGatherThreads;
    hipLaunchKernelGGL(gather_mark_kernel, dim3((unsigned)grid), dim3(kGatherThreads), 0, stream, offset, length,
                       n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap);
}

// One workgroup, two scans.  The bitmap: wpre[w] = set bits in front of word w (wpre[words] = all of them) and
// sel[k] = the k-th set bit, ascending, for k < max_blocks -- nothing is written behind the cap.  The ranges:
// out_off = the exclusive prefix sum of the valid ranges' lengths (n_ranges + 1 entries); it depends on the ranges
// alone.  ctl[0] = the distinct covering blocks; ctl[1] = ENOBUFS when they are more than max_blocks, else ENOSPC
// when the lengths add up to more than out_capacity (or to more than 64 bits hold), else 0.
__global__ __launch_bounds__(kGatherThreads)
void gather_select_kernel(const uint32_t* __restrict__ bitmap, uint32_t n_blocks,
                          const uint64_t* __restrict__ offset, const uint64_t* __restrict__ length, uint32_t n_ranges,
                          uint64_t max_length, uint64_t content_bytes, uint32_t max_blocks, uint64_t out_capacity,
                          uint32_t* __restrict__ wpre, uint32_t* __restrict__ sel, uint64_t* __restrict__ out_off,
                          uint32_t* __restrict__ ctl) {
    __shared__ uint64_t sums[kGatherThreads];
    __shared__ uint32_t cnts[kGatherThreads];
    __shared__ uint32_t wraps[kGatherThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t words = ((uint64_t)n_blocks + 31) / 32;
    const uint64_t per_w = (words + kGatherThreads - 1) / kGatherThreads;
    const uint64_t w0 = t * per_w < words ? t * per_w : words;
    const uint64_t w1 = w0 + per_w < words ? w0 + per_w : words;
    const uint64_t per_r = ((uint64_t)n_ranges + kGatherThreads - 1) / kGatherThreads;
    const uint64_t r0 = t * per_r < n_ranges ? t * per_r : n_ranges;
    const uint64_t r1 = r0 + per_r < n_ranges ? r0 + per_r : n_ranges;
    uint32_t cnt = 0;
    for (uint64_t w = w0; w < w1; w++) { cnt += (uint32_t)__builtin_popcount(bitmap[w]); }
    uint64_t sum = 0;
    uint32_t wrapped = 0;
    for (uint64_t r = r0; r < r1; r++) {
        const uint64_t len = length[r];
        if (gather_range_ok(offset[r], len, max_length, content_bytes)) {
            if (len > ~sum) { wrapped = 1; }
            sum += len;
        }
    }
    cnts[t] = cnt;
    sums[t] = sum;
    wraps[t] = wrapped;
    __syncthreads();
    if (t == 0) {
        uint32_t c = 0, over = 0;
        uint64_t run = 0;
        for (int k = 0; k < kGatherThreads; k++) {
            const uint32_t v = cnts[k];
            cnts[k] = c;
            c += v;
            const uint64_t s = sums[k];
            sums[k] = run;
            if (s > ~run) { over = 1; }
            over |= wraps[k];
            run += s;
        }
        ctl[0] = c;
        ctl[1] = c > max_blocks ? (uint32_t)kErrENOBUFS : (over != 0 || run > out_capacity ? (uint32_t)kErrENOSPC : 0u);
        wpre[words] = c;
        out_off[n_ranges] = run;
    }
    __syncthreads();
    uint32_t k = cnts[t];
    for (uint64_t w = w0; w < w1; w++) {
        uint32_t word = bitmap[w];
        wpre[w] = k;
        while (word != 0) {
            if (k < max_blocks) { sel[k] = (uint32_t)(w * 32) + (uint32_t)__builtin_ctz(word); }
            k++;
            word &= word - 1;
        }
    }
    uint64_t at = sums[t];
    for (uint64_t r = r0; r < r1; r++) {
        const uint64_t len = length[r];
        out_off[r] = at;
        if (gather_range_ok(offset[r], len, max_length, content_bytes)) { at += len; }
    }
}

void launch_gather_select(const uint32_t* bitmap, uint32_t n_blocks, const uint64_t* offset, const uint64_t* length,
                          uint32_t n_ranges, uint64_t max_length, uint64_t content_bytes, uint32_t max_blocks,
                          uint64_t out_capacity, uint32_t* wpre, uint32_t* sel, uint64_t* out_off, uint32_t* ctl,
                          hipStream_t stream) {
    hipLaunchKernelGGL(gather_select_kernel, dim3(1), dim3(kGatherThreads), 0, stream, bitmap, n_blocks, offset,
                       length, n_ranges, max_length, content_bytes, max_blocks, out_capacity, wpre, sel, out_off, ctl);
}

// One lane per range, once the selected blocks lie decoded in the scratch (entry 2k of err and crc is slot k's, as
// frame_open_body<.., true> laid them out).  range_err[r]: EINVAL for an invalid range; the call's status where it
// is not 0; otherwise the first non-zero errno among the covering blocks in ascending order -- what the decoder
// said, or EILSEQ where it was content but the bytes are not the ones the index entry's CRC-32 was taken of.  And
// the range's entry in the copy's work list: where it starts in the decoded blocks (its blocks are consecutive
// slots) and whether it is delivered; destination and length are the caller's out_off.
__global__ __launch_bounds__(kGatherThreads)
void gather_plan_kernel(const uint8_t* __restrict__ frame, const uint64_t* __restrict__ offset,
                        const uint64_t* __restrict__ length, uint32_t n_ranges, uint64_t max_length,
                        uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks,
                        const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                        const int32_t* __restrict__ err, const uint32_t* __restrict__ crc,
                        const int32_t* __restrict__ status, int32_t* __restrict__ range_err,
                        uint64_t* __restrict__ src_off, uint32_t* __restrict__ mask) {
    const uint64_t r = (uint64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    if (r >= n_ranges) { return; }
    const uint64_t off = offset[r], len = length[r];
    if (!gather_range_ok(off, len, max_length, content_bytes)) {
        range_err[r] = kErrEINVAL; src_off[r] = 0; mask[r] = 0;
        return;
    }
    int32_t e = *status;
    uint64_t at = 0;
    const uint64_t first = off >> block_bits;
    if (e == 0 && len > 0 && first < n_blocks) {
        uint64_t last = (off + len - 1) >> block_bits;
        if (last >= n_blocks) { last = (uint64_t)n_blocks - 1; }
        const uint32_t w = bitmap[first >> 5], bit = (uint32_t)first & 31u;
        const uint64_t k0 = wpre[first >> 5] + (uint32_t)__builtin_popcount(w & ((1u << bit) - 1u));
        const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
        for (uint64_t b = first; b <= last && e == 0; b++) {
            const uint64_t k = k0 + (b - first);
            e = err[2 * k];
            if (e == 0 && crc[2 * k] != index[2 * b + 1]) { e = kErrEILSEQ; }
        }
        at = (k0 << block_bits) + (off & ((1ull << block_bits) - 1));
    }
    range_err[r] = e;
    src_off[r] = at;
    mask[r] = e == 0 && len > 0 ? 1u : 0u;
}

void launch_gather_plan(const uint8_t* frame, const uint64_t* offset, const uint64_t* length, uint32_t n_ranges,
                        uint64_t max_length, uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks,
                        const uint32_t* bitmap, const uint32_t* wpre, const int32_t* err, const uint32_t* crc,
                        const int32_t* status, int32_t* range_err, uint64_t* src_off, uint32_t* mask,
                        hipStream_t stream) {
    if (n_ranges == 0) { return; }
    const uint64_t grid = ((uint64_t)n_ranges + kGatherThreads - 1) / kGatherThreads;
    hipLaunchKernelGGL(gather_plan_kernel, dim3((unsigned)grid), dim3(kGatherThreads), 0, stream, frame, offset,
                       length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, wpre, err, crc,
                       status, range_err, src_off, mask);
}

// range_copy_kernel's row load as a function of its own (the kernel above keeps its text, and with it its registers):
// the 16 source bytes at sp of a range [from, src_end), sh = sp & 15: one aligned load when the sides share the
// alignment, two aligned loads joined by a byte shift when both source rows lie inside the range, single bytes otherwise
__device__ __forceinline__ uint4 load_shifted_row(const uint8_t* sp, uint32_t sh, const uint8_t* from,
                                                  const uint8_t* src_end) {
    uint4 v;
    if (sh == 0) {
        v = *reinterpret_cast<const uint4*>(sp);
    } else if (sp - sh >= from && sp - sh + 32 <= src_end) {
        const uint4 a = *reinterpret_cast<const uint4*>(sp - sh);
        const uint4 c = *reinterpret_cast<const uint4*>(sp - sh + 16);
        const uint64_t q0 = (uint64_t)a.x | ((uint64_t)a.y << 32), q1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
        const uint64_t q2 = (uint64_t)c.x | ((uint64_t)c.y << 32), q3 = (uint64_t)c.z | ((uint64_t)c.w << 32);
        const bool up = sh >= 8;
        const uint32_t s = sh & 7u;
        const uint64_t lo = join_bytes(up ? q1 : q0, up ? q2 : q1, s);
        const uint64_t hi = join_bytes(up ? q2 : q1, up ? q3 : q2, s);
        v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
    } else {
        uint32_t w[4] = {0u, 0u, 0u, 0u};           // a source row that is not whole inside the range: byte by byte
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) { w[j >> 2] |= (uint32_t)sp[j] << (8 * (j & 3)); }
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    return v;
}

// range_copy_kernel's work list and rules (nothing outside a source range is read, nothing outside a destination
// range is written, any alignment on either side) for many short ranges: kGatherLanes lanes per range instead of a
// workgroup, so a 256-byte range is one row per lane and a workgroup moves 16 ranges.  No padding.
constexpr uint32_t kGatherLanes = 16;

__global__ __launch_bounds__(kCopyThreads)
void gather_copy_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off,
                        uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_off,
                        const uint64_t* __restrict__ len_off, const uint32_t* __restrict__ mask, uint32_t n_ranges) {
    const uint64_t b = (uint64_t)blockIdx.x * (kCopyThreads / kGatherLanes) + threadIdx.x / kGatherLanes;
    if (b >= n_ranges) { return; }
    if (mask != nullptr && mask[b] == 0) { return; }
    const uint32_t lane = threadIdx.x % kGatherLanes;
    const uint64_t l0 = len_off[b], l1 = len_off[b + 1];
    const uint64_t len = l1 > l0 ? l1 - l0 : 0;
    const uint8_t* const from = src + src_off[b];
    uint8_t* const to = dst + dst_off[b];
    uint64_t head = (16u - (uint32_t)((uintptr_t)to & 15u)) & 15u;     // bytes in front of the first full row
    if (head > len) { head = len; }
    const uint64_t rows = (len - head) / 16;
    const uint64_t tail_at = head + 16 * rows;                         // fewer than 16 bytes behind the last full row
    if (lane < head) { to[lane] = from[lane]; }
    if (lane < len - tail_at) { to[tail_at + lane] = from[tail_at + lane]; }
    const uint8_t* const fb = from + head;
    uint8_t* const tb = to + head;                                     // 16-byte aligned
    const uint32_t sh = (uint32_t)((uintptr_t)fb & 15u);
    for (uint64_t k = lane; k < rows; k += kGatherLanes) {
        *reinterpret_cast<uint4*>(tb + 16 * k) = load_shifted_row(fb + 16 * k, sh, from, from + len);
    }
}

void launch_gather_copy(const uint8_t* src, const uint64_t* src_off, uint8_t* dst, const uint64_t* dst_off,
                        const uint64_t* len_off, const uint32_t* mask, uint32_t n_ranges, hipStream_t stream) {
    if (n_ranges == 0) { return; }
    const uint64_t per = kCopyThreads / kGatherLanes;
    hipLaunchKernelGGL(gather_copy_kernel, dim3((unsigned)(((uint64_t)n_ranges + per - 1) / per)), dim3(kCopyThreads),
                       0, stream, src, src_off, dst, dst_off, len_off, mask, n_ranges);
}

// ---------------------------------------------------------------------------------------- update
// Many byte ranges WRITTEN into a resident frame in one call ("Update"): the distinct covering
// blocks are decoded into slots as a gather decodes them, patched, checksummed and encoded again, every other stream
// is carried over as it lies.  mark -> select -> update_plan -> update_caps -> open for a list -> the decode chain ->
// update_verdict -> the patch (either range copy) -> crc32 -> the encoder over the slots -> frame_merge_index -> crc32
// and seal of the new index -> frame_splice.
constexpr int kErrERANGE = 34, kErrENODATA = 61;   // <errno.h>, checked in abi.hip

// One lane per range, before the frame is opened (validity needs the ranges alone): range_err[r] = EINVAL or 0, and
// the range's entry in the patch copy's work list -- from data + data_off[r] (len_off = data_off: an invalid range
// has length 0 there) to its place in the slots: its covering blocks are consecutive slots, so it lies in one piece
// at (slot of its first block << block_bits) + offset mod 2^block_bits.  flags[0] (zero at the start) becomes 1 when
// any range is invalid.
__global__ __launch_bounds__(kGatherThreads)
void update_plan_kernel(const uint64_t* __restrict__ offset, const uint64_t* __restrict__ length, uint32_t n_ranges,
                        uint64_t max_length, uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks,
                        const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                        const uint64_t* __restrict__ data_off, int32_t* __restrict__ range_err,
                        uint64_t* __restrict__ src_off, uint64_t* __restrict__ dst_off, uint32_t* __restrict__ mask,
                        uint32_t* __restrict__ flags) {
    const uint64_t r = (uint64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    if (r >= n_ranges) { return; }
    const uint64_t off = offset[r], len = length[r];
    if (!gather_range_ok(off, len, max_length, content_bytes)) {
        range_err[r] = kErrEINVAL; src_off[r] = 0; dst_off[r] = 0; mask[r] = 0;
        flags[0] = 1u;                             // every writer writes the same word
        return;
    }
    uint64_t at = 0;
    const uint64_t first = off >> block_bits;
    if (len > 0 && first < n_blocks) {
        const uint32_t w = bitmap[first >> 5], bit = (uint32_t)first & 31u;
        const uint64_t k0 = wpre[first >> 5] + (uint32_t)__builtin_popcount(w & ((1u << bit) - 1u));
        at = (k0 << block_bits) + (off & ((1ull << block_bits) - 1));
    }
    range_err[r] = 0;
    src_off[r] = data_off[r];
    dst_off[r] = at;
    mask[r] = len > 0 ? 1u : 0u;
}

// One lane: what the open kernel takes as the verdict on the request, in the call's order.  ctl[1] arrives as
// gather_select_kernel left it (ENOBUFS, or ENOSPC with the data's size as the capacity) and leaves as EINVAL for a
// frame whose win_bits is not the caller's (ctl[2] = 1: the frame's own status, no block counted), else ERANGE, else
// ENOBUFS, else ENODATA, else 0.
__global__ __launch_bounds__(64)
void update_caps_kernel(const uint8_t* __restrict__ frame, uint32_t win_bits, const uint32_t* __restrict__ flags,
                        uint32_t* __restrict__ ctl) {
    if (threadIdx.x != 0) { return; }
    const uint32_t c = ctl[1];
    const bool other = frame[5] != win_bits;
    ctl[1] = other ? (uint32_t)kErrEINVAL : flags[0] != 0 ? (uint32_t)kErrERANGE
             : c == (uint32_t)kErrENOBUFS ? c : c != 0 ? (uint32_t)kErrENODATA : 0u;
    ctl[2] = other ? 1u : 0u;
}

// One workgroup, once the touched blocks lie decoded in their slots (entry 2k of err and crc is slot k's): *status
// stays what the open kernel said, else becomes the first non-zero errno among the touched blocks in ascending order --
// the decoder's, or EILSEQ where the bytes are not the ones the index entry's CRC-32 was taken of.  With any status
// everything behind is switched off: mask[] of the patch copy is cleared and the encoder's blocks are empty.  Else
// enc_in_off[k] = k << block_bits for the slots in use, the end of the last one (the only one that can be the ragged
// last block) behind them.  slab_off[k] = k * slab_bytes either way (m + 1 entries each).
__global__ __launch_bounds__(256)
void update_verdict_kernel(const uint8_t* __restrict__ frame, const uint32_t* __restrict__ sel,
                           const uint32_t* __restrict__ ctl, uint32_t max_blocks, const int32_t* __restrict__ err,
                           const uint32_t* __restrict__ crc, uint32_t block_bits, uint64_t content_bytes,
                           uint64_t slab_bytes, uint32_t n_ranges, int32_t* __restrict__ status,
                           uint32_t* __restrict__ blocks_encoded, uint32_t* __restrict__ mask,
                           uint64_t* __restrict__ enc_in_off, uint64_t* __restrict__ slab_off) {
    __shared__ uint32_t first_bad[256];
    __shared__ int32_t verdict;
    const uint32_t t = threadIdx.x;
    const uint32_t count = *status == 0 ? ctl[0] : 0u;         // (<= max_blocks: the verdict on the cap was 0)
    const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
    uint32_t mine = 0xFFFFFFFFu;
    for (uint64_t k = t; k < count; k += 256) {
        if (err[2 * k] != 0 || crc[2 * k] != index[2 * (uint64_t)sel[k] + 1]) { mine = (uint32_t)k; break; }
    }
    first_bad[t] = mine;
    __syncthreads();
    if (t == 0) {
        uint32_t bad = 0xFFFFFFFFu;
        for (int k = 0; k < 256; k++) { bad = first_bad[k] < bad ? first_bad[k] : bad; }
        int32_t st = *status;
        if (st == 0 && bad != 0xFFFFFFFFu) { st = err[2 * (uint64_t)bad] != 0 ? err[2 * (uint64_t)bad] : kErrEILSEQ; }
        *status = st;
        if (ctl[2] != 0) { *blocks_encoded = 0u; }
        verdict = st;
    }
    __syncthreads();
    const bool ok = verdict == 0;
    const uint64_t bb = 1ull << block_bits;
    const uint64_t end = ok && count > 0 ? (uint64_t)(count - 1) * bb + block_len(sel[count - 1], bb, content_bytes) : 0;
    for (uint64_t k = t; k <= max_blocks; k += 256) {
        enc_in_off[k] = !ok ? 0 : k < count ? k * bb : end;
        slab_off[k] = k * slab_bytes;
    }
    if (!ok) {
        for (uint64_t r = t; r < n_ranges; r += 256) { mask[r] = 0u; }
    }
}

void launch_update_plan(const uint64_t* offset, const uint64_t* length, uint32_t n_ranges, uint64_t max_length,
                        uint64_t content_bytes, uint32_t block_bits, uint32_t n_blocks, const uint32_t* bitmap,
                        const uint32_t* wpre, const uint64_t* data_off, int32_t* range_err, uint64_t* src_off,
                        uint64_t* dst_off, uint32_t* mask, const uint8_t* frame, uint32_t win_bits, uint32_t* flags,
                        uint32_t* ctl, hipStream_t stream) {
#ifdef SQZ_WAVE_EMU
    flags[0] = 0u;
#else
    (void)hipMemsetAsync(flags, 0, 4, stream);
#endif
    if (n_ranges > 0) {
        const uint64_t grid = ((uint64_t)n_ranges + kGatherThreads - 1) / kGatherThreads;
        hipLaunchKernelGGL(update_plan_kernel, dim3((unsigned)grid), dim3(kGatherThreads), 0, stream, offset, length,
                           n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, wpre, data_off, range_err,
                           src_off, dst_off, mask, flags);
    }
    hipLaunchKernelGGL(update_caps_kernel, dim3(1), dim3(64), 0, stream, frame, win_bits, flags, ctl);
}

void launch_update_verdict(const uint8_t* frame, const uint32_t* sel, const uint32_t* ctl, uint32_t max_blocks,
                           const int32_t* err, const uint32_t* crc, uint32_t block_bits, uint64_t content_bytes,
                           uint64_t slab_bytes, uint32_t n_ranges, int32_t* status, uint32_t* blocks_encoded,
                           uint32_t* mask, uint64_t* enc_in_off, uint64_t* slab_off, hipStream_t stream) {
    hipLaunchKernelGGL(update_verdict_kernel, dim3(1), dim3(256), 0, stream, frame, sel, ctl, max_blocks, err, crc,
                       block_bits, content_bytes, slab_bytes, n_ranges, status, blocks_encoded, mask, enc_in_off, slab_off);
}

// where a segment of the new payload comes from: bits 62..63 of its seg_src word, the offset below them
constexpr uint64_t kSegOld = 0, kSegSlab = 1ull << 62, kSegSlot = 2ull << 62, kSegOffMask = (1ull << 62) - 1;

// One workgroup, the scans shaped as in frame_index_body: the index of the new frame merged from the old entries and
// the encoder's results.  Block b is touched iff its bit is set in bitmap; its slot k (wpre, as in the open kernel) has
// its new stream in slab k (out_bytes[k], enc_err[k]) and its patched content's CRC-32 in crc_new[k]; in a frame whose
// version stores blocks it is stored by frame_index_body's rule (block_stored).  A kept block keeps its entry.  Both
// the old and the new shares are scanned, which gives every block its place in either payload.
// *status arrives as update_verdict_kernel left it.  Non-zero: *frame_bytes_out = 0, idx_off = {0, 0}, an empty segment
// table, nothing else.  Else the first encoder errno in ascending order (or EINVAL for a size no entry holds), else
// E2BIG when the new frame does not fit capacity (*frame_bytes_out = what it takes) -- again nothing of the frame is
// written and the table is empty.  Else header (the old one's fields, the new payload_bytes, index_crc left to
// frame_seal_kernel), index, the old record (kDict) and the padding, idx_off = the index's range for its checksum, and
// the segment table of frame_splice_kernel for the count = ctl[0] touched blocks:
//     segment 2k      the kept streams in front of touched block sel[k] (behind sel[k - 1]), from the old frame
//     segment 2k + 1  block sel[k]: its slab, or its slot when it is stored (seg_len = its content's bytes; the share
//                     is that rounded up to 8)
//     segment 2 count the kept streams behind the last touched block; segments up to 2 max_blocks are empty.
// seg_dst (2 max_blocks + 2 entries, ascending): where a segment starts in the new frame -- the next entry is its end;
// seg_src, seg_len (2 max_blocks + 1): its source (kSeg*) and how many source bytes there are (all ones: as many as
// the segment takes).  A kept run's old offset is the old scan at its first block: no array of n_blocks words.
template <bool kDict>
__device__ __forceinline__
void frame_merge_index_body(const uint8_t* __restrict__ old, uint32_t n_blocks, uint64_t content_bytes,
                            const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                            const uint32_t* __restrict__ ctl, uint32_t max_blocks,
                            const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ enc_err,
                            const uint32_t* __restrict__ crc_new, uint64_t slab_bytes, uint8_t* __restrict__ frame,
                            uint64_t capacity, uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src,
                            uint64_t* __restrict__ seg_len, uint64_t* __restrict__ idx_off,
                            uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status) {
    __shared__ uint64_t sums_old[256];
    __shared__ uint64_t sums_new[256];
    __shared__ int32_t first_err[256];
    __shared__ int32_t verdict;
    __shared__ uint64_t new_end;
    const uint32_t t = threadIdx.x;
    const uint64_t segments = 2 * (uint64_t)max_blocks + 1;
    const uint64_t record = kDict ? 8 : 0;
    const uint64_t payload_off = (32 + 8 * (uint64_t)n_blocks + record + 15) & ~(uint64_t)15;
    if (*status != 0) {                            // (uniform: every lane reads the same word)
        for (uint64_t j = t; j <= segments; j += 256) {
            seg_dst[j] = 0;
            if (j < segments) { seg_src[j] = 0; seg_len[j] = 0; }
        }
        if (t == 0) { *frame_bytes_out = 0; idx_off[0] = 0; idx_off[1] = 0; }
        return;
    }
    // the open kernel has passed this header: its fields are in range
    const uint32_t* const old_index = reinterpret_cast<const uint32_t*>(old + 32);
    const uint32_t block_bits = old[6];
    const bool bit31 = kDict || old[4] == 2;                       // an entry's bit 31 is the stored bit
    const bool store = kDict ? (old[7] & kFrameStored) != 0 : old[4] == 2;
    const uint32_t words_mask = bit31 ? ~kStoredBit : 0xFFFFFFFFu;
    const uint64_t most_words = bit31 ? 0x7FFFFFFFull : 0xFFFFFFFFull;
    const uint64_t bb = 1ull << block_bits;
    const uint32_t count = ctl[0];
    const uint64_t per = ((uint64_t)n_blocks + 255) / 256;
    const uint64_t b0 = t * per < n_blocks ? t * per : n_blocks;
    const uint64_t b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    uint64_t sum_old = 0, sum_new = 0;
    int32_t bad = 0;
    for (uint64_t b = b0; b < b1; b++) {
        const uint64_t share_old = (uint64_t)(old_index[2 * b] & words_mask) * 8;
        uint64_t share_new = share_old;
        const uint32_t w = bitmap[b >> 5], bit = (uint32_t)b & 31u;
        if (((w >> bit) & 1u) != 0) {
            const uint64_t k = wpre[b >> 5] + (uint32_t)__builtin_popcount(w & ((1u << bit) - 1u));
            const uint64_t v = out_bytes[k];
            if (bad == 0 && enc_err[k] != 0) { bad = enc_err[k]; }
            if (bad == 0 && ((v & 7u) != 0 || (v >> 3) > most_words)) { bad = kErrEINVAL; }
            share_new = store ? payload_share(v, block_len(b, bb, content_bytes)) : v;
        }
        sum_old += share_old;
        sum_new += share_new;
    }
    sums_old[t] = sum_old;
    sums_new[t] = sum_new;
    first_err[t] = bad;
    __syncthreads();
    if (t == 0) {
        uint64_t run_old = 0, run_new = 0;
        int32_t st = 0;
        for (int k = 0; k < 256; k++) {
            const uint64_t vo = sums_old[k], vn = sums_new[k];
            sums_old[k] = run_old; sums_new[k] = run_new;
            run_old += vo; run_new += vn;
            if (st == 0) { st = first_err[k]; }
        }
        const uint64_t frame_bytes = payload_off + run_new;
        if (st == 0 && frame_bytes > capacity) { st = kErrE2BIG; }
        verdict = st;
        new_end = frame_bytes;
        *status = st;
        *frame_bytes_out = st == 0 || st == kErrE2BIG ? frame_bytes : 0;
        idx_off[0] = st == 0 ? 32 : 0;
        idx_off[1] = st == 0 ? 32 + 8 * (uint64_t)n_blocks + record : 0;
        if (st == 0) {
            const uint32_t* const oh = reinterpret_cast<const uint32_t*>(old);
            uint32_t* const h = reinterpret_cast<uint32_t*>(frame);
            h[0] = oh[0]; h[1] = oh[1];                            // magic; version, win_bits, block_bits, flags
            h[2] = (uint32_t)content_bytes; h[3] = (uint32_t)(content_bytes >> 32);
            h[4] = (uint32_t)run_new; h[5] = (uint32_t)(run_new >> 32);
            h[6] = n_blocks;
            h[7] = 0u;                                             // index_crc: frame_seal_kernel
            const uint32_t* const old_behind = oh + 8 + 2 * (uint64_t)n_blocks;
            uint32_t* const behind = h + 8 + 2 * (uint64_t)n_blocks;
            if (kDict) {
                behind[0] = old_behind[0]; behind[1] = old_behind[1];
                if ((n_blocks & 1u) == 0) { behind[2] = 0u; behind[3] = 0u; }
            } else if ((n_blocks & 1u) != 0) { behind[0] = 0u; behind[1] = 0u; }
            seg_dst[0] = payload_off; seg_src[0] = kSegOld | payload_off; seg_len[0] = ~(uint64_t)0;
        }
    }
    __syncthreads();
    if (verdict != 0) {
        for (uint64_t j = t; j <= segments; j += 256) {
            seg_dst[j] = 0;
            if (j < segments) { seg_src[j] = 0; seg_len[j] = 0; }
        }
        return;
    }
    uint32_t* const index = reinterpret_cast<uint32_t*>(frame + 32);
    uint64_t at_old = payload_off + sums_old[t], at_new = payload_off + sums_new[t];
    for (uint64_t b = b0; b < b1; b++) {
        const uint32_t e = old_index[2 * b];
        const uint64_t share_old = (uint64_t)(e & words_mask) * 8;
        uint64_t share_new = share_old;
        const uint32_t w = bitmap[b >> 5], bit = (uint32_t)b & 31u;
        if (((w >> bit) & 1u) != 0) {
            const uint64_t k = wpre[b >> 5] + (uint32_t)__builtin_popcount(w & ((1u << bit) - 1u));
            const uint64_t v = out_bytes[k];
            const uint64_t len = block_len(b, bb, content_bytes);
            const bool st = store && block_stored(v, len);
            share_new = store ? payload_share(v, len) : v;
            index[2 * b] = (uint32_t)(share_new >> 3) | (st ? kStoredBit : 0u);
            index[2 * b + 1] = crc_new[k];
            seg_dst[2 * k + 1] = at_new;
            seg_src[2 * k + 1] = st ? kSegSlot | (k * bb) : kSegSlab | (k * slab_bytes);
            seg_len[2 * k + 1] = st ? len : share_new;
            seg_dst[2 * k + 2] = at_new + share_new;               // the kept run behind it: the old frame's bytes
            seg_src[2 * k + 2] = kSegOld | (at_old + share_old);
            seg_len[2 * k + 2] = ~(uint64_t)0;
        } else {
            index[2 * b] = e;
            index[2 * b + 1] = old_index[2 * b + 1];
        }
        at_old += share_old;
        at_new += share_new;
    }
    // the end of the last kept run, and the empty segments behind the count
    for (uint64_t j = 2 * (uint64_t)count + 1 + t; j <= segments; j += 256) {
        seg_dst[j] = new_end;
        if (j < segments) { seg_src[j] = 0; seg_len[j] = 0; }
    }
}

__global__ __launch_bounds__(256)
void frame_merge_index_kernel(const uint8_t* __restrict__ old, uint32_t n_blocks, uint64_t content_bytes,
                              const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                              const uint32_t* __restrict__ ctl, uint32_t max_blocks,
                              const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ enc_err,
                              const uint32_t* __restrict__ crc_new, uint64_t slab_bytes, uint8_t* __restrict__ frame,
                              uint64_t capacity, uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src,
                              uint64_t* __restrict__ seg_len, uint64_t* __restrict__ idx_off,
                              uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status) {
    frame_merge_index_body<false>(old, n_blocks, content_bytes, bitmap, wpre, ctl, max_blocks, out_bytes, enc_err, crc_new,
                                  slab_bytes, frame, capacity, seg_dst, seg_src, seg_len, idx_off, frame_bytes_out, status);
}

__global__ __launch_bounds__(256)
void frame_merge_index_v3_kernel(const uint8_t* __restrict__ old, uint32_t n_blocks, uint64_t content_bytes,
                                 const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ wpre,
                                 const uint32_t* __restrict__ ctl, uint32_t max_blocks,
                                 const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ enc_err,
                                 const uint32_t* __restrict__ crc_new, uint64_t slab_bytes, uint8_t* __restrict__ frame,
                                 uint64_t capacity, uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src,
                                 uint64_t* __restrict__ seg_len, uint64_t* __restrict__ idx_off,
                                 uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status) {
    frame_merge_index_body<true>(old, n_blocks, content_bytes, bitmap, wpre, ctl, max_blocks, out_bytes, enc_err, crc_new,
                                 slab_bytes, frame, capacity, seg_dst, seg_src, seg_len, idx_off, frame_bytes_out, status);
}

void launch_frame_merge_index(const uint8_t* old, uint32_t n_blocks, uint64_t content_bytes, bool dict,
                              const uint32_t* bitmap, const uint32_t* wpre, const uint32_t* ctl, uint32_t max_blocks,
                              const uint64_t* out_bytes, const int32_t* enc_err, const uint32_t* crc_new,
                              uint64_t slab_bytes, uint8_t* frame, uint64_t capacity, uint64_t* seg_dst, uint64_t* seg_src,
                              uint64_t* seg_len, uint64_t* idx_off, uint64_t* frame_bytes_out, int32_t* status,
                              hipStream_t stream) {
    if (dict) {
        hipLaunchKernelGGL(frame_merge_index_v3_kernel, dim3(1), dim3(256), 0, stream, old, n_blocks, content_bytes, bitmap,
                           wpre, ctl, max_blocks, out_bytes, enc_err, crc_new, slab_bytes, frame, capacity, seg_dst, seg_src,
                           seg_len, idx_off, frame_bytes_out, status);
    } else {
        hipLaunchKernelGGL(frame_merge_index_kernel, dim3(1), dim3(256), 0, stream, old, n_blocks, content_bytes, bitmap,
                           wpre, ctl, max_blocks, out_bytes, enc_err, crc_new, slab_bytes, frame, capacity, seg_dst, seg_src,
                           seg_len, idx_off, frame_bytes_out, status);
    }
}

// The payload of the new frame in one pass, partitioned by DESTINATION: a workgroup takes kSpliceChunk bytes of it
// (grid-stride behind the launch's workgroups), finds the first segment that reaches into its chunk by bisection of
// seg_dst and copies the segments' intersections with the chunk until the chunk ends.  A 500 MB kept run between a few
// thousand touched blocks is shared by as many workgroups as it has chunks; range_copy_kernel over the runs would give
// every run the same few.  Every segment starts and ends on a multiple of 8 bytes in the destination, its source
// offset is one as well, the payload starts on a multiple of 16 and so does every chunk: a destination row of 16 bytes
// lies in one chunk and in at most two segments.  A row inside a segment is one aligned 16-byte store of one aligned
// 16-byte load (both sides agree mod 16) or of two aligned 8-byte loads joined (they differ by 8: both halves are the
// segment's own, so nothing outside a source is read).  A row whose halves belong to two segments is written once, by the segment that
// holds its lower half, which fetches the upper half from the next segment that is not empty; only where the payload
// itself ends in mid-row is a store 8 bytes.  Source bytes a segment does not have (seg_len: a stored ragged last
// block's padding) are zeros.  Nothing outside [seg_dst[0], seg_dst[segments]) is written.
constexpr uint64_t kSpliceChunk = 32768;
constexpr unsigned kSpliceMaxGroups = 2048;

// 8 source bytes at p (8-byte aligned) of which only the first `have` exist: the others are zeros
__device__ __forceinline__ uint64_t splice_load8(const uint8_t* p, uint64_t have) {
    if (have >= 8) { return *reinterpret_cast<const uint64_t*>(p); }
    uint64_t v = 0;
    for (uint32_t j = 0; j < have; j++) { v |= (uint64_t)p[j] << (8 * j); }
    return v;
}

struct SpliceSource { const uint8_t* from; uint64_t have; };       // a segment's first source byte, and how many there are

__device__ __forceinline__ SpliceSource splice_source(const uint8_t* old, const uint8_t* slabs, const uint8_t* slots,
                                                      uint64_t word, uint64_t len, uint64_t room) {
    const uint64_t sel = word & ~kSegOffMask;
    SpliceSource s;
    s.from = (sel == kSegOld ? old : sel == kSegSlab ? slabs : slots) + (word & kSegOffMask);
    s.have = len < room ? len : room;
    return s;
}

__global__ __launch_bounds__(kCopyThreads)
void frame_splice_kernel(const uint8_t* __restrict__ old, const uint8_t* __restrict__ slabs,
                         const uint8_t* __restrict__ slots, uint8_t* __restrict__ dst,
                         const uint64_t* __restrict__ seg_dst, const uint64_t* __restrict__ seg_src,
                         const uint64_t* __restrict__ seg_len, uint32_t segments) {
    const uint64_t base = seg_dst[0], end = seg_dst[segments];
    if (end <= base) { return; }
    const uint64_t chunks = (end - base + kSpliceChunk - 1) / kSpliceChunk;
    const uint32_t tid = threadIdx.x;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t c0 = base + c * kSpliceChunk;
        const uint64_t c1 = end - c0 > kSpliceChunk ? c0 + kSpliceChunk : end;
        uint32_t lo = 0, hi = segments - 1;                        // the first segment that ends behind c0
        while (lo < hi) {
            const uint32_t mid = (lo + hi) / 2;
            if (seg_dst[mid + 1] > c0) { hi = mid; } else { lo = mid + 1; }
        }
        for (uint32_t j = lo; j < segments; j++) {
            const uint64_t s0 = seg_dst[j], s1 = seg_dst[j + 1];
            if (s0 >= c1) { break; }
            if (s1 <= s0) { continue; }
            const uint64_t a = s0 > c0 ? s0 : c0, b = s1 < c1 ? s1 : c1;
            const SpliceSource src = splice_source(old, slabs, slots, seg_src[j], seg_len[j], s1 - s0);
            for (uint64_t r = (a & ~(uint64_t)15) + 16 * (uint64_t)tid; r < b; r += 16 * (uint64_t)kCopyThreads) {
                if (r < a) { continue; }                           // the lower half is the segment's in front: its row
                const uint8_t* const sp = src.from + (r - s0);
                const uint64_t have = src.have > r - s0 ? src.have - (r - s0) : 0;
                if (r + 16 <= b) {
                    uint4 v;
                    if (have >= 16 && ((uintptr_t)sp & 15u) == 0) {
                        v = *reinterpret_cast<const uint4*>(sp);
                    } else if (have >= 16) {                       // sp is 8 mod 16: two aligned halves, both the segment's
                        const uint64_t q0 = *reinterpret_cast<const uint64_t*>(sp);
                        const uint64_t q1 = *reinterpret_cast<const uint64_t*>(sp + 8);
                        v.x = (uint32_t)q0; v.y = (uint32_t)(q0 >> 32); v.z = (uint32_t)q1; v.w = (uint32_t)(q1 >> 32);
                    } else {
                        const uint64_t q0 = splice_load8(sp, have), q1 = splice_load8(sp + 8, have > 8 ? have - 8 : 0);
                        v.x = (uint32_t)q0; v.y = (uint32_t)(q0 >> 32); v.z = (uint32_t)q1; v.w = (uint32_t)(q1 >> 32);
                    }
                    *reinterpret_cast<uint4*>(dst + r) = v;
                    continue;
                }
                // the segment ends in mid-row (never the chunk, unless the payload does): the upper half is the first
                // 8 bytes of the next segment that is not empty
                const uint64_t q0 = splice_load8(sp, have);
                uint32_t n = j + 1;
                while (n < segments && seg_dst[n + 1] <= seg_dst[n]) { n++; }
                if (n < segments) {
                    const SpliceSource nx = splice_source(old, slabs, slots, seg_src[n], seg_len[n], seg_dst[n + 1] - seg_dst[n]);
                    const uint64_t q1 = splice_load8(nx.from, nx.have);
                    uint4 v;
                    v.x = (uint32_t)q0; v.y = (uint32_t)(q0 >> 32); v.z = (uint32_t)q1; v.w = (uint32_t)(q1 >> 32);
                    *reinterpret_cast<uint4*>(dst + r) = v;
                } else {
                    *reinterpret_cast<uint64_t*>(dst + r) = q0;
                }
            }
        }
    }
}

// most_bytes: the most the new payload can be (the launch's size; the table on the device says what it is)
void launch_frame_splice(const uint8_t* old, const uint8_t* slabs, const uint8_t* slots, uint8_t* dst,
                         const uint64_t* seg_dst, const uint64_t* seg_src, const uint64_t* seg_len, uint32_t max_blocks,
                         uint64_t most_bytes, hipStream_t stream) {
    uint64_t groups = (most_bytes + kSpliceChunk - 1) / kSpliceChunk;
    if (groups > kSpliceMaxGroups) { groups = kSpliceMaxGroups; }
    if (groups < 1) { groups = 1; }
    hipLaunchKernelGGL(frame_splice_kernel, dim3((unsigned)groups), dim3(kCopyThreads), 0, stream, old, slabs, slots, dst,
                       seg_dst, seg_src, seg_len, 2 * max_blocks + 1);
}

// the same kernel over a table of `segments` segments (an append's: one kept run and its new blocks)
void launch_frame_splice_segments(const uint8_t* old, const uint8_t* slabs, const uint8_t* slots, uint8_t* dst,
                                  const uint64_t* seg_dst, const uint64_t* seg_src, const uint64_t* seg_len,
                                  uint32_t segments, uint64_t most_bytes, hipStream_t stream) {
    uint64_t groups = (most_bytes + kSpliceChunk - 1) / kSpliceChunk;
    if (groups > kSpliceMaxGroups) { groups = kSpliceMaxGroups; }
    if (groups < 1) { groups = 1; }
    hipLaunchKernelGGL(frame_splice_kernel, dim3((unsigned)groups), dim3(kCopyThreads), 0, stream, old, slabs, slots, dst,
                       seg_dst, seg_src, seg_len, segments);
}

// ---------------------------------------------------------------------------------------- append
// data_bytes more content behind a resident frame in one call ("Append"): a NEW frame of
// content || data.  The host knows content_bytes (C), data_bytes (A) and block_bits (b), and with them t = C mod 2^b
// (the bytes of a ragged last block), whether that block is touched (t > 0 and A > 0), keep = n_blocks - (touched ? 1 :
// 0) blocks whose entries and streams are carried over, m = ceil((t + A) / 2^b) blocks to encode (0 for A = 0) and
// n' = keep + m: no device count sizes a launch.  append_plan -> open for a list of at most one block -> the decode
// chain (touched only) -> append_verdict -> the data into the staging area (range_copy_kernel, one range) -> crc32 ->
// the encoder over the staging area -> frame_append_index -> crc32 and seal of the new index -> frame_splice.
//
// One lane per bitmap word and one behind them: what the open kernel takes for a list -- bit n_blocks - 1 set iff the
// last block is touched, wpre (no bit in front of any word, wpre[words] = the count), sel[0], ctl[0] = the count -- and
// ctl[1], the verdict on the request: EINVAL for a frame whose win_bits is not the caller's, else 0.
__global__ __launch_bounds__(kGatherThreads)
void append_plan_kernel(const uint8_t* __restrict__ frame, uint32_t n_blocks, uint64_t content_bytes,
                        uint64_t data_bytes, uint32_t block_bits, uint32_t win_bits, uint32_t* __restrict__ bitmap,
                        uint32_t* __restrict__ wpre, uint32_t* __restrict__ sel, uint32_t* __restrict__ ctl) {
    const uint64_t words = ((uint64_t)n_blocks + 31) / 32;
    const uint64_t w = (uint64_t)blockIdx.x * kGatherThreads + threadIdx.x;
    const bool touched = n_blocks > 0 && data_bytes > 0 && (content_bytes & ((1ull << block_bits) - 1)) != 0;
    if (w < words) {
        const uint32_t last = n_blocks - 1u;
        bitmap[w] = touched && w == (last >> 5) ? 1u << (last & 31u) : 0u;
        wpre[w] = 0u;
    } else if (w == words) {
        wpre[words] = touched ? 1u : 0u;
        if (touched) { sel[0] = n_blocks - 1u; }
        ctl[0] = touched ? 1u : 0u;
        ctl[1] = frame[5] != win_bits ? (uint32_t)kErrEINVAL : 0u;
    }
}

// One workgroup, once the touched block (if any) lies decoded at the head of the staging area (entry 0 of err and crc
// is its).  *blocks_encoded = 0 for a status of the open kernel's (the frame's own, or the other win_bits), else m.
// *status stays what the open kernel said, else becomes the touched block's errno -- the decoder's, or EILSEQ where the
// bytes are not the ones the index entry's CRC-32 was taken of.  The staging copy's one-range work list (copy: 5 x
// uint64 as launch_frame_read_plan's -- src_off = copy[0] = 0, dst_off = copy + 1 = where the data starts, len_off =
// copy + 2 = {0, data_bytes}, mask = (uint32_t*)(copy + 4)) is masked out under any status, and the encoder's blocks
// are empty then (enc_in_off all zeros); else enc_in_off[k] = k << block_bits, the last block's end at t + data_bytes.
// slab_off[k] = k * slab_bytes either way (m + 1 entries each).
__global__ __launch_bounds__(256)
void append_verdict_kernel(const uint8_t* __restrict__ frame, uint32_t n_blocks, const uint32_t* __restrict__ ctl,
                           const int32_t* __restrict__ err, const uint32_t* __restrict__ crc, uint32_t block_bits,
                           uint64_t content_bytes, uint64_t data_bytes, uint32_t m, uint64_t slab_bytes,
                           int32_t* __restrict__ status, uint32_t* __restrict__ blocks_encoded,
                           uint64_t* __restrict__ copy, uint64_t* __restrict__ enc_in_off,
                           uint64_t* __restrict__ slab_off) {
    __shared__ int32_t verdict;
    const uint32_t t = threadIdx.x;
    const uint64_t bb = 1ull << block_bits;
    const uint64_t head = data_bytes > 0 ? content_bytes & (bb - 1) : 0;      // the touched block's bytes in front of the data
    if (t == 0) {
        int32_t st = *status;
        *blocks_encoded = st != 0 ? 0u : m;
        if (st == 0 && ctl[0] != 0) {
            const uint32_t want = reinterpret_cast<const uint32_t*>(frame + 32)[2 * (uint64_t)(n_blocks - 1u) + 1];
            st = err[0] != 0 ? err[0] : crc[0] != want ? kErrEILSEQ : 0;
        }
        *status = st;
        verdict = st;
        copy[0] = 0; copy[1] = head;
        copy[2] = 0; copy[3] = data_bytes;
        *reinterpret_cast<uint32_t*>(copy + 4) = st == 0 && data_bytes > 0 ? 1u : 0u;
    }
    __syncthreads();
    const bool ok = verdict == 0;
    const uint64_t end = head + data_bytes;
    for (uint64_t k = t; k <= m; k += 256) {
        enc_in_off[k] = !ok ? 0 : k * bb < end ? k * bb : end;
        slab_off[k] = k * slab_bytes;
    }
}

// One workgroup of 256, the scans shaped as in frame_merge_index_body: the index of the new frame from the old entries
// of the keep blocks in front and the encoder's results for the m blocks behind them.  Each lane takes
// ceil(n' / 256) consecutive blocks of the NEW frame.  A block below keep takes its entry from the old index; its share
// feeds the old scan as well, whose total is the kept run's length.  A block at or above keep takes slot k = block -
// keep: its stream in slab k (out_bytes[k], enc_err[k]), its content's CRC-32 in crc_new[k], stored by
// frame_index_body's rule where the version stores blocks, its content then at k << block_bits of the staging area.
// *status arrives as append_verdict_kernel left it.  Non-zero: *frame_bytes_out = 0, idx_off = {0, 0}, an empty segment
// table, nothing else.  Else the first encoder errno in ascending order (or EINVAL for a size no entry holds), else
// E2BIG when the new frame does not fit capacity (*frame_bytes_out = what it takes) -- again nothing of the frame is
// written and the table is empty.  Else the header (the old magic, version, win_bits, block_bits and flags; the new
// content_bytes, payload_bytes and n_blocks; index_crc left to frame_seal_kernel), the n' entries, the old record
// (kDict), the padding up to payload_off = pad16(32 + 8 n' (+ 8)), idx_off = the index's range for its checksum, and
// the table of frame_splice_kernel, m + 1 segments (seg_dst m + 2 entries, ascending; seg_src, seg_len m + 1):
//     segment 0       the kept run, from the old frame's payload_off to the new one's (both multiples of 16); as long
//                     as the old scan says, so the touched block's old stream is left behind
//     segment k + 1   new block k: its slab, or its place in the staging area when it is stored (seg_len = its content's
//                     bytes; the share is that rounded up to 8)
template <bool kDict>
__device__ __forceinline__
void frame_append_index_body(const uint8_t* __restrict__ old, uint32_t n_blocks, uint64_t content_bytes,
                             uint64_t data_bytes, uint32_t m, const uint64_t* __restrict__ out_bytes,
                             const int32_t* __restrict__ enc_err, const uint32_t* __restrict__ crc_new,
                             uint64_t slab_bytes, uint8_t* __restrict__ frame, uint64_t capacity,
                             uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src,
                             uint64_t* __restrict__ seg_len, uint64_t* __restrict__ idx_off,
                             uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status) {
    __shared__ uint64_t sums_old[256];
    __shared__ uint64_t sums_new[256];
    __shared__ int32_t first_err[256];
    __shared__ int32_t verdict;
    const uint32_t t = threadIdx.x;
    const uint64_t segments = (uint64_t)m + 1;
    if (*status != 0) {                            // (uniform: every lane reads the same word)
        for (uint64_t j = t; j <= segments; j += 256) {
            seg_dst[j] = 0;
            if (j < segments) { seg_src[j] = 0; seg_len[j] = 0; }
        }
        if (t == 0) { *frame_bytes_out = 0; idx_off[0] = 0; idx_off[1] = 0; }
        return;
    }
    // the open kernel has passed this header: its fields are in range
    const uint32_t* const old_index = reinterpret_cast<const uint32_t*>(old + 32);
    const uint32_t block_bits = old[6];
    const bool bit31 = kDict || old[4] == 2;                       // an entry's bit 31 is the stored bit
    const bool store = kDict ? (old[7] & kFrameStored) != 0 : old[4] == 2;
    const uint32_t words_mask = bit31 ? ~kStoredBit : 0xFFFFFFFFu;
    const uint64_t most_words = bit31 ? 0x7FFFFFFFull : 0xFFFFFFFFull;
    const uint64_t bb = 1ull << block_bits;
    const uint64_t record = kDict ? 8 : 0;
    const bool touched = n_blocks > 0 && data_bytes > 0 && (content_bytes & (bb - 1)) != 0;
    const uint64_t keep = (uint64_t)n_blocks - (touched ? 1 : 0);
    const uint64_t n_new = keep + m;                               // (fits 32 bits: the caller saw to it)
    const uint64_t new_content = content_bytes + data_bytes;
    const uint64_t old_payload_off = (32 + 8 * (uint64_t)n_blocks + record + 15) & ~(uint64_t)15;
    const uint64_t payload_off = (32 + 8 * n_new + record + 15) & ~(uint64_t)15;
    const uint64_t per = (n_new + 255) / 256;
    const uint64_t b0 = t * per < n_new ? t * per : n_new;
    const uint64_t b1 = b0 + per < n_new ? b0 + per : n_new;
    uint64_t sum_old = 0, sum_new = 0;
    int32_t bad = 0;
    for (uint64_t b = b0; b < b1; b++) {
        if (b < keep) {
            const uint64_t share = (uint64_t)(old_index[2 * b] & words_mask) * 8;
            sum_old += share;
            sum_new += share;
        } else {
            const uint64_t k = b - keep;
            const uint64_t v = out_bytes[k];
            if (bad == 0 && enc_err[k] != 0) { bad = enc_err[k]; }
            if (bad == 0 && ((v & 7u) != 0 || (v >> 3) > most_words)) { bad = kErrEINVAL; }
            sum_new += store ? payload_share(v, block_len(b, bb, new_content)) : v;
        }
    }
    sums_old[t] = sum_old;
    sums_new[t] = sum_new;
    first_err[t] = bad;
    __syncthreads();
    if (t == 0) {
        uint64_t run_old = 0, run_new = 0;
        int32_t st = 0;
        for (int k = 0; k < 256; k++) {
            const uint64_t vn = sums_new[k];
            run_old += sums_old[k];
            sums_new[k] = run_new;
            run_new += vn;
            if (st == 0) { st = first_err[k]; }
        }
        const uint64_t frame_bytes = payload_off + run_new;
        if (st == 0 && frame_bytes > capacity) { st = kErrE2BIG; }
        verdict = st;
        *status = st;
        *frame_bytes_out = st == 0 || st == kErrE2BIG ? frame_bytes : 0;
        idx_off[0] = st == 0 ? 32 : 0;
        idx_off[1] = st == 0 ? 32 + 8 * n_new + record : 0;
        if (st == 0) {
            const uint32_t* const oh = reinterpret_cast<const uint32_t*>(old);
            uint32_t* const h = reinterpret_cast<uint32_t*>(frame);
            h[0] = oh[0]; h[1] = oh[1];                            // magic; version, win_bits, block_bits, flags
            h[2] = (uint32_t)new_content; h[3] = (uint32_t)(new_content >> 32);
            h[4] = (uint32_t)run_new; h[5] = (uint32_t)(run_new >> 32);
            h[6] = (uint32_t)n_new;
            h[7] = 0u;                                             // index_crc: frame_seal_kernel
            const uint32_t* const old_behind = oh + 8 + 2 * (uint64_t)n_blocks;
            uint32_t* const behind = h + 8 + 2 * n_new;
            if (kDict) {
                behind[0] = old_behind[0]; behind[1] = old_behind[1];
                if ((n_new & 1u) == 0) { behind[2] = 0u; behind[3] = 0u; }
            } else if ((n_new & 1u) != 0) { behind[0] = 0u; behind[1] = 0u; }
            seg_dst[0] = payload_off; seg_src[0] = kSegOld | old_payload_off; seg_len[0] = run_old;
            seg_dst[segments] = frame_bytes;                       // (m = 0: the kept run's end)
        }
    }
    __syncthreads();
    if (verdict != 0) {
        for (uint64_t j = t; j <= segments; j += 256) {
            seg_dst[j] = 0;
            if (j < segments) { seg_src[j] = 0; seg_len[j] = 0; }
        }
        return;
    }
    uint32_t* const index = reinterpret_cast<uint32_t*>(frame + 32);
    uint64_t at = payload_off + sums_new[t];
    for (uint64_t b = b0; b < b1; b++) {
        uint64_t share;
        if (b < keep) {
            const uint32_t e = old_index[2 * b];
            share = (uint64_t)(e & words_mask) * 8;
            index[2 * b] = e;
            index[2 * b + 1] = old_index[2 * b + 1];
        } else {
            const uint64_t k = b - keep;
            const uint64_t v = out_bytes[k];
            const uint64_t len = block_len(b, bb, new_content);
            const bool st = store && block_stored(v, len);
            share = store ? payload_share(v, len) : v;
            index[2 * b] = (uint32_t)(share >> 3) | (st ? kStoredBit : 0u);
            index[2 * b + 1] = crc_new[k];
            seg_dst[k + 1] = at;
            seg_src[k + 1] = st ? kSegSlot | (k * bb) : kSegSlab | (k * slab_bytes);
            seg_len[k + 1] = st ? len : share;
        }
        at += share;
    }
}

__global__ __launch_bounds__(256)
void frame_append_index_kernel(const uint8_t* __restrict__ old, uint32_t n_blocks, uint64_t content_bytes,
                               uint64_t data_bytes, uint32_t m, const uint64_t* __restrict__ out_bytes,
                               const int32_t* __restrict__ enc_err, const uint32_t* __restrict__ crc_new,
                               uint64_t slab_bytes, uint8_t* __restrict__ frame, uint64_t capacity,
                               uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src,
                               uint64_t* __restrict__ seg_len, uint64_t* __restrict__ idx_off,
                               uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status) {
    frame_append_index_body<false>(old, n_blocks, content_bytes, data_bytes, m, out_bytes, enc_err, crc_new, slab_bytes,
                                   frame, capacity, seg_dst, seg_src, seg_len, idx_off, frame_bytes_out, status);
}

__global__ __launch_bounds__(256)
void frame_append_index_v3_kernel(const uint8_t* __restrict__ old, uint32_t n_blocks, uint64_t content_bytes,
                                  uint64_t data_bytes, uint32_t m, const uint64_t* __restrict__ out_bytes,
                                  const int32_t* __restrict__ enc_err, const uint32_t* __restrict__ crc_new,
                                  uint64_t slab_bytes, uint8_t* __restrict__ frame, uint64_t capacity,
                                  uint64_t* __restrict__ seg_dst, uint64_t* __restrict__ seg_src,
                                  uint64_t* __restrict__ seg_len, uint64_t* __restrict__ idx_off,
                                  uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status) {
    frame_append_index_body<true>(old, n_blocks, content_bytes, data_bytes, m, out_bytes, enc_err, crc_new, slab_bytes,
                                  frame, capacity, seg_dst, seg_src, seg_len, idx_off, frame_bytes_out, status);
}

void launch_append_plan(const uint8_t* frame, uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                        uint32_t block_bits, uint32_t win_bits, uint32_t* bitmap, uint32_t* wpre, uint32_t* sel,
                        uint32_t* ctl, hipStream_t stream) {
    const uint64_t words = ((uint64_t)n_blocks + 31) / 32;
    const uint64_t grid = (words + 1 + kGatherThreads - 1) / kGatherThreads;
    hipLaunchKernelGGL(append_plan_kernel, dim3((unsigned)grid), dim3(kGatherThreads), 0, stream, frame, n_blocks,
                       content_bytes, data_bytes, block_bits, win_bits, bitmap, wpre, sel, ctl);
}

void launch_append_verdict(const uint8_t* frame, uint32_t n_blocks, const uint32_t* ctl, const int32_t* err,
                           const uint32_t* crc, uint32_t block_bits, uint64_t content_bytes, uint64_t data_bytes,
                           uint32_t m, uint64_t slab_bytes, int32_t* status, uint32_t* blocks_encoded, uint64_t* copy,
                           uint64_t* enc_in_off, uint64_t* slab_off, hipStream_t stream) {
    hipLaunchKernelGGL(append_verdict_kernel, dim3(1), dim3(256), 0, stream, frame, n_blocks, ctl, err, crc, block_bits,
                       content_bytes, data_bytes, m, slab_bytes, status, blocks_encoded, copy, enc_in_off, slab_off);
}

void launch_frame_append_index(const uint8_t* old, uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                               uint32_t m, bool dict, const uint64_t* out_bytes, const int32_t* enc_err,
                               const uint32_t* crc_new, uint64_t slab_bytes, uint8_t* frame, uint64_t capacity,
                               uint64_t* seg_dst, uint64_t* seg_src, uint64_t* seg_len, uint64_t* idx_off,
                               uint64_t* frame_bytes_out, int32_t* status, hipStream_t stream) {
    if (dict) {
        hipLaunchKernelGGL(frame_append_index_v3_kernel, dim3(1), dim3(256), 0, stream, old, n_blocks, content_bytes,
                           data_bytes, m, out_bytes, enc_err, crc_new, slab_bytes, frame, capacity, seg_dst, seg_src,
                           seg_len, idx_off, frame_bytes_out, status);
    } else {
        hipLaunchKernelGGL(frame_append_index_kernel, dim3(1), dim3(256), 0, stream, old, n_blocks, content_bytes,
                           data_bytes, m, out_bytes, enc_err, crc_new, slab_bytes, frame, capacity, seg_dst, seg_src,
                           seg_len, idx_off, frame_bytes_out, status);
    }
}

// ---------------------------------------------------------------------------------------- batches of frames
// k frames in one call ("Batches of frames"): one workgroup per frame does what the one
// workgroup of a single call does, around the same frame_index_body / frame_open_body, so that the number of
// launches does not depend on k.  The frame's workgroup sums its own index as well -- every lane the entries of its
// share, joined in LDS -- so there is neither a checksum launch per frame nor one that reads the payload between two
// indexes, and the seal needs no launch of its own.
namespace {

constexpr int kFramesThreads = 256;

// x^(64 n): the n index entries (8 bytes each) one lane has summed
__device__ __forceinline__ uint32_t xpow64_lane(uint64_t n) {
    uint32_t p = kCrcOne;
    for (int j = 0; n != 0; j++, n >>= 1) {
        if ((n & 1u) != 0) { p = gf_mul(p, kCrcTab.pow2[(j + 6) & 31]); }
    }
    return p;
}

// The whole workgroup: lane t brings r = the register after its `count` entries from state 0 (no initial value, no
// final xor) -- the lanes' shares lie in ascending order -- and every lane gets zlib's crc32 of all entries; *power
// = x^(8 * their bytes).  (r, p) pairs join by (rA, pA) . (rB, pB) = (rA pB ^ rB, pA pB), in a tree over LDS.
__device__ __forceinline__ uint32_t index_crc_workgroup(uint32_t r, uint64_t count, uint32_t* power) {
    __shared__ uint32_t join_r[kFramesThreads];
    __shared__ uint32_t join_p[kFramesThreads];
    const uint32_t t = threadIdx.x;
    join_r[t] = r;
    join_p[t] = xpow64_lane(count);
    for (uint32_t s = 1; s < kFramesThreads; s <<= 1) {
        __syncthreads();
        if ((t & (2 * s - 1)) == 0) {
            const uint32_t pb = join_p[t + s];
            join_r[t] = gf_mul(join_r[t], pb) ^ join_r[t + s];
            join_p[t] = gf_mul(join_p[t], pb);
        }
    }
    __syncthreads();
    const uint32_t p = join_p[0];
    const uint32_t c = join_r[0] ^ gf_mul(0xFFFFFFFFu, p) ^ 0xFFFFFFFFu;
    __syncthreads();                               // the arrays may be written again
    *power = p;
    return c;
}

// sqz_frame_bound_ex, rounded up to 16: what frame f of a batch may take of d_frames
__device__ __forceinline__ uint64_t frames_slot_bytes(uint64_t content_bytes, uint32_t block_bits, bool store) {
    const uint64_t bb = 1ull << block_bits, full = content_bytes >> block_bits, tail = content_bytes & (bb - 1);
    const uint64_t n = full + (tail != 0 ? 1 : 0);
    const uint64_t payload_off = (32 + 8 * n + 15) & ~(uint64_t)15;
    const uint64_t payload = store ? (content_bytes + 7) & ~(uint64_t)7
                                   : full * ((2 * bb + 1024 + 7) & ~(uint64_t)7) +
                                     (tail != 0 ? (2 * tail + 1024 + 7) & ~(uint64_t)7 : 0);
    return (payload_off + payload + 15) & ~(uint64_t)15;
}

// exclusive scans over the k frames of a batch by one workgroup: lane t sums its share, lane 0 the 256 shares
template <int kN>
__device__ __forceinline__ void frames_scan_shares(uint64_t (&mine)[kN], uint64_t (*shares)[kFramesThreads]) {
    const uint32_t t = threadIdx.x;
    for (int j = 0; j < kN; j++) { shares[j][t] = mine[j]; }
    __syncthreads();
    if (t == 0) {
        for (int j = 0; j < kN; j++) {
            uint64_t run = 0;
            for (int q = 0; q < kFramesThreads; q++) { const uint64_t v = shares[j][q]; shares[j][q] = run; run += v; }
        }
    }
    __syncthreads();
    for (int j = 0; j < kN; j++) { mine[j] = shares[j][t]; }
}

} // namespace

// encode, one workgroup: in_at (where frame f's content starts in d_in), frame_at (where its frame starts in
// d_frames: the bounds, each rounded up to 16) and base (its first block in the batch's arrays), k + 1 entries each
__global__ __launch_bounds__(kFramesThreads)
void frames_encode_scan_kernel(const uint64_t* __restrict__ content_bytes, uint32_t k, uint32_t block_bits,
                               uint32_t flags, uint64_t* __restrict__ in_at, uint64_t* __restrict__ frame_at,
                               uint32_t* __restrict__ base) {
    __shared__ uint64_t shares[3][kFramesThreads];
    const uint32_t t = threadIdx.x;
    const bool store = (flags & kFrameStored) != 0;
    const uint64_t per = ((uint64_t)k + kFramesThreads - 1) / kFramesThreads;
    const uint64_t f0 = t * per < k ? t * per : k;
    const uint64_t f1 = f0 + per < k ? f0 + per : k;
    const uint64_t bb = 1ull << block_bits;
    uint64_t at[3] = {0, 0, 0};
    for (uint64_t f = f0; f < f1; f++) {
        const uint64_t c = content_bytes[f];
        at[0] += c;
        at[1] += frames_slot_bytes(c, block_bits, store);
        at[2] += (c >> block_bits) + ((c & (bb - 1)) != 0 ? 1 : 0);
    }
    frames_scan_shares(at, shares);
    for (uint64_t f = f0; f < f1; f++) {
        const uint64_t c = content_bytes[f];
        in_at[f] = at[0]; frame_at[f] = at[1]; base[f] = (uint32_t)at[2];
        at[0] += c;
        at[1] += frames_slot_bytes(c, block_bits, store);
        at[2] += (c >> block_bits) + ((c & (bb - 1)) != 0 ? 1 : 0);
    }
    if (f1 == k && (f0 < f1 || t == 0)) { in_at[k] = at[0]; frame_at[k] = at[1]; base[k] = (uint32_t)at[2]; }
}

// encode, workgroup f: frame_plan_kernel for frame f's blocks, at their place in the batch's arrays (the contents lie
// back to back, so a frame's last block ends where the next frame's first begins); the last frame closes both arrays
__global__ __launch_bounds__(kFramesThreads)
void frames_plan_kernel(const uint64_t* __restrict__ content_bytes, const uint64_t* __restrict__ in_at,
                        const uint32_t* __restrict__ base, uint32_t k, uint32_t block_bits, uint64_t slab_bytes,
                        uint64_t* __restrict__ in_off, uint64_t* __restrict__ slab_off) {
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint64_t g0 = base[f], n = base[f + 1] - base[f], at = in_at[f], c = content_bytes[f];
    for (uint64_t b = threadIdx.x; b < n; b += kFramesThreads) {
        in_off[g0 + b] = at + (b << block_bits);   // b < n: inside the content
        slab_off[g0 + b] = (g0 + b) * slab_bytes;
    }
    if (f == k - 1 && threadIdx.x == 0) { in_off[g0 + n] = at + c; slab_off[g0 + n] = (g0 + n) * slab_bytes; }
}

// encode, workgroup f: frame_index_body for frame f at d_frames + frame_at[f] over its slice of the batch's arrays, then
// the seal (frame_seal_kernel's arithmetic over the entries this workgroup has just written) and the dense offsets
// once more, absolute in d_frames, for one compaction and one copy of stored blocks over the whole batch.
// dense_rel: total blocks + k entries (frame f's n + 1 at base[f] + f), the body's own offsets from the frame's start
__global__ __launch_bounds__(kFramesThreads)
void frames_index_kernel(const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ err,
                         const uint32_t* __restrict__ crc, const uint64_t* __restrict__ content_bytes,
                         const uint64_t* __restrict__ frame_at, const uint32_t* __restrict__ base, uint32_t k,
                         uint32_t win_bits, uint32_t block_bits, uint32_t flags, uint8_t* __restrict__ frames,
                         uint64_t* __restrict__ copy_bytes, uint64_t* __restrict__ dense_rel,
                         uint64_t* __restrict__ dense_off, uint32_t* __restrict__ stored,
                         uint64_t* __restrict__ frame_bytes_out, int32_t* __restrict__ status_out) {
    __shared__ uint64_t idx_range[2];              // the body's range for a checksum launch: not needed here
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint32_t t = threadIdx.x;
    const uint64_t g0 = base[f];
    const uint32_t n = base[f + 1] - base[f];
    const uint64_t at = frame_at[f], capacity = frame_at[f + 1] - at, content = content_bytes[f];
    uint8_t* const frame = frames + at;
    uint64_t* const rel = dense_rel + g0 + f;
    uint32_t* const mask = (flags & kFrameStored) != 0 ? stored + g0 : nullptr;
    frame_index_body<false>(out_bytes + g0, err + g0, crc + g0, n, content, win_bits, block_bits, frame, capacity,
                            copy_bytes + g0, rel, idx_range, frame_bytes_out + f, status_out + f,
                            flags & kFrameStored, mask, 0u, nullptr);
    __syncthreads();                               // the body's writes, lane 0's status among them
    const bool ok = status_out[f] == 0;
    const uint64_t per = ((uint64_t)n + 255) / 256;            // the body's shares: a lane sums the entries it wrote
    const uint64_t b0 = t * per < n ? t * per : n;
    const uint64_t b1 = b0 + per < n ? b0 + per : n;
    const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
    uint32_t r = 0;
    for (uint64_t b = b0; b < b1; b++) {
        dense_off[g0 + b] = ok ? at + rel[b] : 0;
        if (ok) { r = crc_word(crc_word(r ^ index[2 * b]) ^ index[2 * b + 1]); }
    }
    uint32_t power;
    const uint32_t idx_crc = index_crc_workgroup(r, b1 - b0, &power);
    if (ok && t == 0) { reinterpret_cast<uint32_t*>(frame)[7] = gf_mul(crc32_small(frame, 28), power) ^ idx_crc; }
    if (f == k - 1 && t == 0) { dense_off[g0 + n] = ok ? at + rel[n] : 0; }
}

// decode, one workgroup: base[f] = the blocks in front of frame f (k + 1 entries); frame f's entries start at
// base[f] + f
__global__ __launch_bounds__(kFramesThreads)
void frames_decode_scan_kernel(const sqz_frames_item* __restrict__ items, uint32_t k, uint32_t* __restrict__ base) {
    __shared__ uint64_t shares[1][kFramesThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t per = ((uint64_t)k + kFramesThreads - 1) / kFramesThreads;
    const uint64_t f0 = t * per < k ? t * per : k;
    const uint64_t f1 = f0 + per < k ? f0 + per : k;
    uint64_t at[1] = {0};
    for (uint64_t f = f0; f < f1; f++) { at[0] += items[f].n_blocks; }
    frames_scan_shares(at, shares);
    for (uint64_t f = f0; f < f1; f++) { base[f] = (uint32_t)at[0]; at[0] += items[f].n_blocks; }
    if (f1 == k && (f0 < f1 || t == 0)) { base[k] = (uint32_t)at[0]; }
}

// decode, workgroup f: the checksum of frame f's index, frame_open_body (versions 1 and 2, all blocks) over the
// frame's n + 1 entries at base[f] + f, then the entries once more: in_off absolute in d_frames, out_off from out_base
// (out_at[0]; the decode kernels address one uint32 slot per output byte by it), and skip.  Entry n is the pseudo-entry
// frame_open_list_kernel has per slot: it reaches from the end of this frame's payload to the next frame's first
// stream and is switched off.  A refused frame: its status, and every entry empty and switched off.  The last frame
// closes both arrays.  The caller made sure that avail covers header and index.
__global__ __launch_bounds__(kFramesThreads)
void frames_open_kernel(const uint8_t* __restrict__ frames, const sqz_frames_item* __restrict__ items,
                        const uint32_t* __restrict__ base, uint32_t k, uint64_t out_base,
                        uint64_t* __restrict__ in_off, uint64_t* __restrict__ out_off, uint32_t* __restrict__ skip,
                        uint32_t* __restrict__ stored, int32_t* __restrict__ status_out) {
    __shared__ uint32_t idx_crc;
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint32_t t = threadIdx.x;
    const uint64_t at = items[f].frame_at, avail = items[f].avail, content = items[f].content_bytes;
    const uint64_t to = items[f].out_at - out_base;
    const uint32_t n = items[f].n_blocks;
    const uint64_t e0 = (uint64_t)base[f] + f;
    const uint8_t* const frame = frames + at;
    const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
    const uint64_t per = ((uint64_t)n + 255) / 256;
    const uint64_t b0 = t * per < n ? t * per : n;
    const uint64_t b1 = b0 + per < n ? b0 + per : n;
    uint32_t r = 0;
    for (uint64_t b = b0; b < b1; b++) { r = crc_word(crc_word(r ^ index[2 * b]) ^ index[2 * b + 1]); }
    uint32_t power;
    const uint32_t c = index_crc_workgroup(r, b1 - b0, &power);
    if (t == 0) { idx_crc = c; }
    __syncthreads();
    frame_open_body<false>(frame, avail, n, content, 0u, n, &idx_crc, in_off + e0, out_off + e0, status_out + f,
                           stored + e0, 0u, nullptr, 0u);
    __syncthreads();
    const bool ok = status_out[f] == 0;
    for (uint64_t j = t; j <= n; j += kFramesThreads) {
        in_off[e0 + j] = ok ? at + in_off[e0 + j] : at;
        out_off[e0 + j] = ok ? to + out_off[e0 + j] : to;
        const uint32_t raw = j < n ? stored[e0 + j] : 0u;      // the body: all zeros on a refusal
        stored[e0 + j] = raw;
        skip[e0 + j] = ok && j < n ? raw : 1u;
    }
    __syncthreads();
    if (f == k - 1 && t == 0) { in_off[e0 + n + 1] = in_off[e0 + n]; out_off[e0 + n + 1] = out_off[e0 + n]; }
}

// decode, workgroup f: frame_verify_kernel for frame f.  err: the decode chain's, one per ENTRY (block b of frame f at
// base[f] + f + b); err_out: the caller's, one per BLOCK (at base[f] + b) -- the frame's status where it was refused,
// EILSEQ where the decoder was content but the bytes are not the ones that were checksummed, else what the decoder said
__global__ __launch_bounds__(kFramesThreads)
void frames_verify_kernel(const uint8_t* __restrict__ frames, const sqz_frames_item* __restrict__ items,
                          const uint32_t* __restrict__ base, uint32_t k, const uint32_t* __restrict__ crc,
                          const int32_t* __restrict__ status, const int32_t* __restrict__ err,
                          int32_t* __restrict__ err_out) {
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint64_t g0 = base[f], e0 = g0 + f;
    const uint32_t n = items[f].n_blocks;
    const int32_t st = status[f];
    const uint32_t* const index = reinterpret_cast<const uint32_t*>(frames + items[f].frame_at + 32);
    for (uint64_t b = threadIdx.x; b < n; b += kFramesThreads) {
        int32_t e = st;
        if (st == 0) {
            e = err[e0 + b];
            if (e == 0 && crc[e0 + b] != index[2 * b + 1]) { e = kErrEILSEQ; }
        }
        err_out[g0 + b] = e;
    }
}

// ---- the flavours that know version 4: elem[f] = frame f's element size (2, 4 or 8), 0 an unshuffled frame.  Siblings
// of the kernels above, which stay as they are; what a frame's workgroup does is the same body either way.

// sqz_frame_bound_shuf where the frame is shuffled (the record's 8 bytes in front of the padding), sqz_frame_bound_ex
// where it is not, rounded up to 16
__device__ __forceinline__ uint64_t frames_slot_bytes_v4(uint64_t content_bytes, uint32_t block_bits, bool store,
                                                         uint32_t elem_bytes) {
    const uint64_t bb = 1ull << block_bits, full = content_bytes >> block_bits, tail = content_bytes & (bb - 1);
    const uint64_t n = full + (tail != 0 ? 1 : 0);
    const uint64_t payload_off = (32 + 8 * n + (elem_bytes != 0 ? 8 : 0) + 15) & ~(uint64_t)15;
    const uint64_t payload = store ? (content_bytes + 7) & ~(uint64_t)7
                                   : full * ((2 * bb + 1024 + 7) & ~(uint64_t)7) +
                                     (tail != 0 ? (2 * tail + 1024 + 7) & ~(uint64_t)7 : 0);
    return (payload_off + payload + 15) & ~(uint64_t)15;
}

// encode_scan over those bounds
__global__ __launch_bounds__(kFramesThreads)
void frames_encode_scan_v4_kernel(const uint64_t* __restrict__ content_bytes, const uint32_t* __restrict__ elem,
                                  uint32_t k, uint32_t block_bits, uint32_t flags, uint64_t* __restrict__ in_at,
                                  uint64_t* __restrict__ frame_at, uint32_t* __restrict__ base) {
    __shared__ uint64_t shares[3][kFramesThreads];
    const uint32_t t = threadIdx.x;
    const bool store = (flags & kFrameStored) != 0;
    const uint64_t per = ((uint64_t)k + kFramesThreads - 1) / kFramesThreads;
    const uint64_t f0 = t * per < k ? t * per : k;
    const uint64_t f1 = f0 + per < k ? f0 + per : k;
    const uint64_t bb = 1ull << block_bits;
    uint64_t at[3] = {0, 0, 0};
    for (uint64_t f = f0; f < f1; f++) {
        const uint64_t c = content_bytes[f];
        at[0] += c;
        at[1] += frames_slot_bytes_v4(c, block_bits, store, elem[f]);
        at[2] += (c >> block_bits) + ((c & (bb - 1)) != 0 ? 1 : 0);
    }
    frames_scan_shares(at, shares);
    for (uint64_t f = f0; f < f1; f++) {
        const uint64_t c = content_bytes[f];
        in_at[f] = at[0]; frame_at[f] = at[1]; base[f] = (uint32_t)at[2];
        at[0] += c;
        at[1] += frames_slot_bytes_v4(c, block_bits, store, elem[f]);
        at[2] += (c >> block_bits) + ((c & (bb - 1)) != 0 ? 1 : 0);
    }
    if (f1 == k && (f0 < f1 || t == 0)) { in_at[k] = at[0]; frame_at[k] = at[1]; base[k] = (uint32_t)at[2]; }
}

// plan, and the element size of every block of the batch for shuffle_ranges_kernel
__global__ __launch_bounds__(kFramesThreads)
void frames_plan_v4_kernel(const uint64_t* __restrict__ content_bytes, const uint32_t* __restrict__ elem,
                           const uint64_t* __restrict__ in_at, const uint32_t* __restrict__ base, uint32_t k,
                           uint32_t block_bits, uint64_t slab_bytes, uint64_t* __restrict__ in_off,
                           uint64_t* __restrict__ slab_off, uint32_t* __restrict__ blk_elem) {
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint64_t g0 = base[f], n = base[f + 1] - base[f], at = in_at[f], c = content_bytes[f];
    const uint32_t e = elem[f];
    for (uint64_t b = threadIdx.x; b < n; b += kFramesThreads) {
        in_off[g0 + b] = at + (b << block_bits);   // b < n: inside the content
        slab_off[g0 + b] = (g0 + b) * slab_bytes;
        blk_elem[g0 + b] = e;
    }
    if (f == k - 1 && threadIdx.x == 0) { in_off[g0 + n] = at + c; slab_off[g0 + n] = (g0 + n) * slab_bytes; }
}

// index: frame_index_body<false, kShuf> by elem[f]; a shuffled frame's checksum takes the record in, which is one more
// 8-byte entry behind the last lane's share
__global__ __launch_bounds__(kFramesThreads)
void frames_index_v4_kernel(const uint64_t* __restrict__ out_bytes, const int32_t* __restrict__ err,
                            const uint32_t* __restrict__ crc, const uint64_t* __restrict__ content_bytes,
                            const uint32_t* __restrict__ elem, const uint64_t* __restrict__ frame_at,
                            const uint32_t* __restrict__ base, uint32_t k, uint32_t win_bits, uint32_t block_bits,
                            uint32_t flags, uint8_t* __restrict__ frames, uint64_t* __restrict__ copy_bytes,
                            uint64_t* __restrict__ dense_rel, uint64_t* __restrict__ dense_off,
                            uint32_t* __restrict__ stored, uint64_t* __restrict__ frame_bytes_out,
                            int32_t* __restrict__ status_out) {
    __shared__ uint64_t idx_range[2];
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint32_t t = threadIdx.x;
    const uint64_t g0 = base[f];
    const uint32_t n = base[f + 1] - base[f];
    const uint64_t at = frame_at[f], capacity = frame_at[f + 1] - at, content = content_bytes[f];
    const uint32_t e = elem[f];                    // the same for the whole workgroup
    uint8_t* const frame = frames + at;
    uint64_t* const rel = dense_rel + g0 + f;
    uint32_t* const mask = (flags & kFrameStored) != 0 ? stored + g0 : nullptr;
    if (e != 0) {
        frame_index_body<false, true>(out_bytes + g0, err + g0, crc + g0, n, content, win_bits, block_bits, frame,
                                      capacity, copy_bytes + g0, rel, idx_range, frame_bytes_out + f, status_out + f,
                                      (flags & kFrameStored) | kFrameShuffle, mask, e, nullptr);
    } else {
        frame_index_body<false>(out_bytes + g0, err + g0, crc + g0, n, content, win_bits, block_bits, frame, capacity,
                                copy_bytes + g0, rel, idx_range, frame_bytes_out + f, status_out + f,
                                flags & kFrameStored, mask, 0u, nullptr);
    }
    __syncthreads();                               // the body's writes, lane 0's status among them
    const bool ok = status_out[f] == 0;
    const uint64_t per = ((uint64_t)n + 255) / 256;
    const uint64_t b0 = t * per < n ? t * per : n;
    const uint64_t b1 = b0 + per < n ? b0 + per : n;
    const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
    uint32_t r = 0;
    uint64_t count = b1 - b0;
    for (uint64_t b = b0; b < b1; b++) {
        dense_off[g0 + b] = ok ? at + rel[b] : 0;
        if (ok) { r = crc_word(crc_word(r ^ index[2 * b]) ^ index[2 * b + 1]); }
    }
    if (e != 0 && t == kFramesThreads - 1) {       // the last share, empty or not, ends where the record begins
        if (ok) { r = crc_word(crc_word(r ^ index[2 * (uint64_t)n]) ^ index[2 * (uint64_t)n + 1]); }
        count += 1;
    }
    uint32_t power;
    const uint32_t idx_crc = index_crc_workgroup(r, count, &power);
    if (ok && t == 0) { reinterpret_cast<uint32_t*>(frame)[7] = gf_mul(crc32_small(frame, 28), power) ^ idx_crc; }
    if (f == k - 1 && t == 0) { dense_off[g0 + n] = ok ? at + rel[n] : 0; }
}

// open: items[f].zero is the caller's element size for frame f.  A version-4 header with one named: frame_open_body's
// version-4 reader with it; a version-4 header with none, or another version with one: EINVAL, nothing of the frame
// behind its header is read; else the reader of versions 1 and 2 as in frames_open_kernel.  ent_elem: the element size
// of every entry for shuffle_ranges_kernel, 0 for the switched-off entry of every frame.
__global__ __launch_bounds__(kFramesThreads)
void frames_open_v4_kernel(const uint8_t* __restrict__ frames, const sqz_frames_item* __restrict__ items,
                           const uint32_t* __restrict__ base, uint32_t k, uint64_t out_base,
                           uint64_t* __restrict__ in_off, uint64_t* __restrict__ out_off, uint32_t* __restrict__ skip,
                           uint32_t* __restrict__ stored, uint32_t* __restrict__ ent_elem,
                           int32_t* __restrict__ status_out) {
    __shared__ uint32_t idx_crc;
    const uint32_t f = blockIdx.x;
    if (f >= k) { return; }
    const uint32_t t = threadIdx.x;
    const uint64_t at = items[f].frame_at, avail = items[f].avail, content = items[f].content_bytes;
    const uint64_t to = items[f].out_at - out_base;
    const uint32_t n = items[f].n_blocks, e = items[f].zero;
    const uint64_t e0 = (uint64_t)base[f] + f;
    const uint8_t* const frame = frames + at;
    const bool v4 = frame[4] == 4;                 // the same for the whole workgroup, like e
    if (v4 != (e != 0)) {
        if (t == 0) { status_out[f] = kErrEINVAL; }
    } else {
        const uint32_t* const index = reinterpret_cast<const uint32_t*>(frame + 32);
        const uint64_t per = ((uint64_t)n + 255) / 256;
        const uint64_t b0 = t * per < n ? t * per : n;
        const uint64_t b1 = b0 + per < n ? b0 + per : n;
        uint32_t r = 0;
        uint64_t count = b1 - b0;
        for (uint64_t b = b0; b < b1; b++) { r = crc_word(crc_word(r ^ index[2 * b]) ^ index[2 * b + 1]); }
        if (v4 && t == kFramesThreads - 1) {       // the record, behind the last share
            r = crc_word(crc_word(r ^ index[2 * (uint64_t)n]) ^ index[2 * (uint64_t)n + 1]);
            count += 1;
        }
        uint32_t power;
        const uint32_t c = index_crc_workgroup(r, count, &power);
        if (t == 0) { idx_crc = c; }
        __syncthreads();
        if (v4) {
            frame_open_body<false, false, true>(frame, avail, n, content, 0u, n, &idx_crc, in_off + e0, out_off + e0,
                                                status_out + f, stored + e0, e, nullptr, 0u);
        } else {
            frame_open_body<false>(frame, avail, n, content, 0u, n, &idx_crc, in_off + e0, out_off + e0, status_out + f,
                                   stored + e0, 0u, nullptr, 0u);
        }
    }
    __syncthreads();
    const bool ok = status_out[f] == 0;
    for (uint64_t j = t; j <= n; j += kFramesThreads) {
        in_off[e0 + j] = ok ? at + in_off[e0 + j] : at;
        out_off[e0 + j] = ok ? to + out_off[e0 + j] : to;
        const uint32_t raw = ok && j < n ? stored[e0 + j] : 0u;
        stored[e0 + j] = raw;
        skip[e0 + j] = ok && j < n ? raw : 1u;
        ent_elem[e0 + j] = j < n ? e : 0u;
    }
    __syncthreads();
    if (f == k - 1 && t == 0) { in_off[e0 + n + 1] = in_off[e0 + n]; out_off[e0 + n + 1] = out_off[e0 + n]; }
}

void launch_frames_encode_scan_v4(const uint64_t* content_bytes, const uint32_t* elem, uint32_t k, uint32_t block_bits,
                                  uint32_t flags, uint64_t* in_at, uint64_t* frame_at, uint32_t* base,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(frames_encode_scan_v4_kernel, dim3(1), dim3(kFramesThreads), 0, stream, content_bytes, elem, k,
                       block_bits, flags, in_at, frame_at, base);
}

void launch_frames_plan_v4(const uint64_t* content_bytes, const uint32_t* elem, const uint64_t* in_at,
                           const uint32_t* base, uint32_t k, uint32_t block_bits, uint64_t slab_bytes, uint64_t* in_off,
                           uint64_t* slab_off, uint32_t* blk_elem, hipStream_t stream) {
    hipLaunchKernelGGL(frames_plan_v4_kernel, dim3(k), dim3(kFramesThreads), 0, stream, content_bytes, elem, in_at, base,
                       k, block_bits, slab_bytes, in_off, slab_off, blk_elem);
}

void launch_frames_index_v4(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc,
                            const uint64_t* content_bytes, const uint32_t* elem, const uint64_t* frame_at,
                            const uint32_t* base, uint32_t k, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                            uint8_t* frames, uint64_t* copy_bytes, uint64_t* dense_rel, uint64_t* dense_off,
                            uint32_t* stored, uint64_t* frame_bytes_out, int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frames_index_v4_kernel, dim3(k), dim3(kFramesThreads), 0, stream, out_bytes, err, crc,
                       content_bytes, elem, frame_at, base, k, win_bits, block_bits, flags, frames, copy_bytes,
                       dense_rel, dense_off, stored, frame_bytes_out, status_out);
}

void launch_frames_open_v4(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                           uint64_t out_base, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                           uint32_t* ent_elem, int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frames_open_v4_kernel, dim3(k), dim3(kFramesThreads), 0, stream, frames, items, base, k,
                       out_base, in_off, out_off, skip, stored, ent_elem, status_out);
}

void launch_frames_encode_scan(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits, uint32_t flags,
                               uint64_t* in_at, uint64_t* frame_at, uint32_t* base, hipStream_t stream) {
    hipLaunchKernelGGL(frames_encode_scan_kernel, dim3(1), dim3(kFramesThreads), 0, stream, content_bytes, k,
                       block_bits, flags, in_at, frame_at, base);
}

void launch_frames_plan(const uint64_t* content_bytes, const uint64_t* in_at, const uint32_t* base, uint32_t k,
                        uint32_t block_bits, uint64_t slab_bytes, uint64_t* in_off, uint64_t* slab_off,
                        hipStream_t stream) {
    hipLaunchKernelGGL(frames_plan_kernel, dim3(k), dim3(kFramesThreads), 0, stream, content_bytes, in_at, base, k,
                       block_bits, slab_bytes, in_off, slab_off);
}

void launch_frames_index(const uint64_t* out_bytes, const int32_t* err, const uint32_t* crc,
                         const uint64_t* content_bytes, const uint64_t* frame_at, const uint32_t* base, uint32_t k,
                         uint32_t win_bits, uint32_t block_bits, uint32_t flags, uint8_t* frames, uint64_t* copy_bytes,
                         uint64_t* dense_rel, uint64_t* dense_off, uint32_t* stored, uint64_t* frame_bytes_out,
                         int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frames_index_kernel, dim3(k), dim3(kFramesThreads), 0, stream, out_bytes, err, crc,
                       content_bytes, frame_at, base, k, win_bits, block_bits, flags, frames, copy_bytes, dense_rel,
                       dense_off, stored, frame_bytes_out, status_out);
}

void launch_frames_decode_scan(const sqz_frames_item* items, uint32_t k, uint32_t* base, hipStream_t stream) {
    hipLaunchKernelGGL(frames_decode_scan_kernel, dim3(1), dim3(kFramesThreads), 0, stream, items, k, base);
}

void launch_frames_open(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                        uint64_t out_base, uint64_t* in_off, uint64_t* out_off, uint32_t* skip, uint32_t* stored,
                        int32_t* status_out, hipStream_t stream) {
    hipLaunchKernelGGL(frames_open_kernel, dim3(k), dim3(kFramesThreads), 0, stream, frames, items, base, k, out_base,
                       in_off, out_off, skip, stored, status_out);
}

void launch_frames_verify(const uint8_t* frames, const sqz_frames_item* items, const uint32_t* base, uint32_t k,
                          const uint32_t* crc, const int32_t* status, const int32_t* err, int32_t* err_out,
                          hipStream_t stream) {
    hipLaunchKernelGGL(frames_verify_kernel, dim3(k), dim3(kFramesThreads), 0, stream, frames, items, base, k, crc,
                       status, err, err_out);
}

} // namespace sqzk
