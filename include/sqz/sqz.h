/* include/sqz/sqz.h -- C ABI of libsqz_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE path of leok7v/sqz: the LZ77 longest-match scan +
 * adaptive-Huffman emit (encode) and its inverse (decode).  C99, plain pointers
 * and sizes; no HIP or torch types appear in any signature (streams and device
 * pointers travel as void*).
 *
 * Four layers, all backed by the same HIP kernels (there is NO CPU fallback:
 * every entry point reports ENODEV when no gfx950 device can be opened):
 *
 *  1. single-stream API with the reference's documented names
 *     (sqz_init / sqz_write_header / sqz_compress / sqz_read_header /
 *      sqz_decompress, `struct sqz`, `sqz_type`, `struct bitstream`):
 *       - names + call shape: /root/reference/shl/README.md:31-62,
 *         /root/reference/README.md:66-131 ("H1" in SURVEY.md section 0)
 *       - behaviour (bit-exact): attic/map_experiment/squeeze.h ("H0"):
 *         compress :319-409, decompress :502-551, header :255-265/:444-456
 *  2. the H0 vtable spelling `squeeze` (squeeze.h:109-131) for callers of the
 *     attic harness (attic/map_experiment/test.c:54-61,114-134)
 *  3. batch API over independent blocks -- the data-parallel hot path:
 *     host-buffer flavour and device-resident flavour (what bench.py times).
 *  4. SQZF frames: one checksummed, seekable artifact for one large buffer, built from
 *     layer 3's streams (this project's container, not the reference's; see below).
 *
 * Errors are the reference's sticky errno integers (squeeze.h:82,224-237;
 * bitstream.h:15,38,74): 0, EINVAL, E2BIG, ENOMEM; plus ENODEV (no GPU) and, for frames,
 * EILSEQ (a checksum does not match).
 */
#ifndef SQZ_AMD_SQZ_H
#define SQZ_AMD_SQZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SQZ_API __attribute__((visibility("default")))
#else
#define SQZ_API
#endif

enum {
    sqz_min_win_bits = 10,  /* squeeze.h:19  squeeze_min_win_bits */
    sqz_max_win_bits = 15,  /* squeeze.h:20  squeeze_max_win_bits */
    sqz_min_len      = 3,   /* squeeze.h:13  squeeze_deflate_len_min */
    sqz_max_len      = 257, /* squeeze.h:15  squeeze_deflate_len_max */
    sqz_header_bits  = 72   /* squeeze.h:255-265: 64 (bytes) + 8 (win_bits) */
};

/* The public constants of the H0 header under the reference's own names (squeeze.h:9-25), same
 * values: what a caller of the `squeeze` vtable compiles against (attic/map_experiment/test.c
 * passes win_bits in [squeeze_min_win_bits, squeeze_max_win_bits] and sizes init_with's block
 * with squeeze_sizeof).                                                                      */
enum {
    squeeze_deflate_sym_min = 257,  /* squeeze.h:10 first length symbol of the literal/length alphabet */
    squeeze_deflate_sym_max = 284,  /* squeeze.h:11 last one                                           */
    squeeze_deflate_pos_max = 29,   /* squeeze.h:12 last distance code                                 */
    squeeze_deflate_len_min = 3,    /* squeeze.h:13 */
    squeeze_deflate_len_max = 257   /* squeeze.h:15 */
};
enum {
    squeeze_min_win_bits = 10,      /* squeeze.h:19 */
    squeeze_max_win_bits = 15,      /* squeeze.h:20 */
    squeeze_min_map_bits = 16,      /* squeeze.h:21 (the map experiment: map_bits != 0 is refused here) */
    squeeze_max_map_bits = 28,      /* squeeze.h:22 */
    squeeze_lit_nyt = squeeze_deflate_sym_max + 1,   /* squeeze.h:23 = 285 */
    squeeze_pos_nyt = squeeze_deflate_pos_max + 1    /* squeeze.h:24 = 30  */
};

/* ------------------------------------------------------------------ */
/* Bit stream: `bitstream` of attic/map_experiment/bitstream.h:7-18, same fields in the same
 * order, so the reference's designated initialisers compile unchanged
 * (attic/map_experiment/test.c:53,110):
 *
 *   memory mode   { .data = buf, .capacity = sizeof buf }            writer -> .bytes produced
 *                 { .data = buf, .bytes = n }                        reader (H0, test.c:110)
 *                 { .data = buf, .capacity = n }                     reader (H1, shl/README.md:47-48)
 *   callback mode { .stream = f, .output = write_file }              writer (bitstream.h:44-48)
 *                 { .stream = f, .input  = read_file  }              reader (bitstream.h:81-85)
 *
 * Callback mode is served by the shim, since a device cannot call the host per word
 * (SURVEY.md section 8b "Ownership"):
 *   writer  the stream is produced on the device into a host buffer, then every 64-bit word
 *           is handed over exactly as bitstream.h:45-47 does: bs->b64 = word, bs->error =
 *           bs->output(bs), bs->bytes += 8 on success, stop at the first error.  Same calls,
 *           same order, same values as the reference makes.
 *   reader  words are pulled with bs->input(bs) (bs->b64 = the word, bitstream.h:83) into a host
 *           buffer and decoded from there.  The reference pulls a word when its bit reader
 *           runs dry; the device decodes a whole buffer at once, so the shim pulls ahead:
 *           4 words first, then twice as many each time the decoder runs dry (E2BIG), decoding
 *           again from the start.  OVER-READ BOUND: the words pulled are at most
 *           max(4, 2 x the words the stream holds), whatever its compression ratio -- the
 *           reference pulls exactly the words the stream holds (bitstream.h:81-85), so a
 *           caller whose source continues behind the stream (another record in the same file)
 *           must re-position the source from bs->read, which IS the reference's figure; a
 *           pulled word cannot be handed back.  A callback error only surfaces if the decoder
 *           needed words beyond it.  bs->read / bs->bits / bs->b64 are left as the reference's
 *           reader would leave them (read = words the DECODER consumed x 8).               */
typedef struct bitstream {
    void*    stream;   /* callback context (bitstream.h:8); exclusive with (data, capacity) */
    uint8_t* data;
    uint64_t capacity; /* data[capacity] */
    uint64_t bytes;    /* bytes written (writer) / available (reader) */
    uint64_t read;     /* bytes consumed by the reader */
    uint64_t b64;      /* bit shifting buffer (bitstream.h:13) */
    int32_t  bits;     /* bit count inside b64 (bitstream.h:14) */
    int32_t  error;    /* sticky errno (bitstream.h:15; errno_t is int) */
    int (*output)(struct bitstream* bs); /* write b64 as 8 bytes (bitstream.h:16) */
    int (*input)(struct bitstream* bs);  /* read b64 as 8 bytes  (bitstream.h:17) */
} bitstream;

/* codec state (squeeze_type, squeeze.h:81-92).  Caller-owned, single-use per stream like the
 * reference's (squeeze.h:333-334 inserts the NYT leaves at the start of every call).  The
 * trees themselves live on the device for the duration of a call; the struct carries what the
 * reference's callers read afterwards: the sticky error (first member, as in the reference)
 * and the bit stream of the last call (`s->bs->bytes`, attic test.c:84).                  */
struct sqz {
    int32_t  error;       /* sticky errno: README.md:126-131, squeeze.h:82 */
    int32_t  device;      /* HIP device ordinal used by the last call, -1 = default */
    uint64_t tokens;      /* LZ77 tokens of the last sqz_compress */
    struct bitstream* bs; /* squeeze.h:89: set by compress / decompress */
    void*    stream;      /* optional hipStream_t the call's copies and kernels are enqueued on; NULL (what
                           * sqz_init / alloc / init_with leave) = a stream of the library's own, one per
                           * call in flight.  Calls from different threads do not serialise on each other:
                           * every call stages through buffers of its own. */
    uint64_t reserved[3];
};
typedef struct sqz sqz_type; /* README.md:128 */

/* squeeze.h:94-107 squeeze_sizeof(map_bits): the size of the block `init_with` takes (squeeze.h:191-199).
 * The reference lays its trees out behind the struct; here they live in the device's LDS for the duration of
 * a call, so the block is the struct.  init_with accepts any size >= this (a caller that kept the reference's
 * larger figure still passes); map_bits must be 0.                                                       */
#define squeeze_sizeof(map_bits) (sizeof(struct sqz))

/* shl/README.md:37-38  `static struct sqz s; sqz_init(&s);` */
SQZ_API void sqz_init(struct sqz* s);

/* shl/README.md:34 spelling (2 arguments).  The H1 source is absent from the
 * reference snapshot, so its framing cannot be pinned: this writes the 64-bit
 * length only, LSB first (the first field of squeeze.h:255-265).            */
SQZ_API void sqz_write_header(struct bitstream* bs, uint64_t bytes);
SQZ_API void sqz_read_header(struct bitstream* bs, uint64_t* bytes);

/* squeeze.h:255-265 / :444-456 framing, pinned by tests/golden: 64 bits of
 * length + 8 bits of win_bits (10..15, else bs->error = EINVAL), LSB first,
 * no alignment before the payload.                                          */
SQZ_API void sqz_write_header_h0(struct bitstream* bs, uint64_t bytes, uint8_t win_bits);
SQZ_API void sqz_read_header_h0(struct bitstream* bs, uint64_t* bytes, uint8_t* win_bits);

/* squeeze.h:319-409.  `window` = 1u << win_bits (2..32768 accepted, like the
 * reference's uint16_t argument; max distance is window-1).  Continues the bit
 * stream wherever sqz_write_header* left it and zero-pads to a 64-bit boundary
 * (bitstream.h:112-114).  Result in s->error (mirrored to bs->error), output
 * size in bs->bytes.  E2BIG when bs->capacity is too small (bitstream.h:38).  In callback
 * mode (bs->data == NULL, bs->output set) every word goes through bs->output.            */
SQZ_API void sqz_compress(struct sqz* s, struct bitstream* bs,
                          const uint8_t* data, size_t bytes, uint32_t window);

/* squeeze.h:502-551.  Decodes exactly `bytes` bytes (taken from the header). */
SQZ_API void sqz_decompress(struct sqz* s, struct bitstream* bs,
                            uint8_t* data, size_t bytes);

/* ------------------------------------------------------------------ */
/* H0 vtable spelling: squeeze.h:109-131.  `map_bits` must be 0 (the map
 * experiment is disabled in the reference's default configuration,
 * attic/map_experiment/test.c:30-31) -- anything else is EINVAL / NULL.     */
typedef struct sqz squeeze_type;
typedef struct {
    squeeze_type* (*alloc)(uint8_t map_bits);
    int  (*init_with)(squeeze_type* s, void* memory, size_t size, uint8_t map_bits);
    void (*write_header)(bitstream* bs, uint64_t bytes, uint8_t win_bits);
    void (*compress)(squeeze_type* s, bitstream* bs,
                     const uint8_t* data, size_t bytes, uint16_t window);
    void (*read_header)(bitstream* bs, uint64_t* bytes, uint8_t* win_bits);
    void (*decompress)(squeeze_type* s, bitstream* bs, uint8_t* data, size_t bytes);
    void (*free)(squeeze_type* s);
} squeeze_interface;
SQZ_API extern squeeze_interface squeeze;

/* ------------------------------------------------------------------ */
/* Batch API: n independent blocks, each a self-contained stream with fresh
 * trees (squeeze.h:333-336), payload only (no header), every output a multiple
 * of 8 bytes.  Block b reads  in[in_off[b] .. in_off[b+1])  and writes at most
 * out_off[b+1]-out_off[b] bytes at out + out_off[b]; the size goes to
 * out_bytes[b], the errno to err[b].  Offsets arrays have n+1 entries.
 * out_off[b] must be a multiple of 8.  Only out[out_off[b] .. + out_bytes[b]) is written.     */

/* worst-case compressed size of one block of `bytes` bytes (multiple of 8) */
SQZ_API uint64_t sqz_bound(uint64_t bytes);

/* File-mode bit streams (attic/map_experiment/test.c:39-42,98-101; bitstream.h `.stream`,
 * `.output`, `.input`): the reference hands every 64-bit word of the stream to
 * fwrite(&b64, 8, 1, f) / fread(&b64, 8, 1, f), i.e. in HOST byte order, while a memory-mode
 * stream holds the words most-significant byte first.  This converts one image into the
 * other (the operation is its own inverse; on a big-endian host it is a copy): write
 * out[] with fwrite to get the file the reference's harness writes, or pass a file's bytes
 * through it to get the stream sqz_decompress / sqz_decode_blocks read.  `bytes` must be a
 * multiple of 8 (every stream is, bitstream.h:112-114); in == out is allowed.
 * Returns 0 or EINVAL.  Host code: no device is touched.                              */
SQZ_API int sqz_file_words(const uint8_t* in, uint64_t bytes, uint8_t* out);

/* host buffers in, host buffers out (H2D + kernels + D2H inside) */
SQZ_API int sqz_encode_blocks(const uint8_t* in, const uint64_t* in_off, uint32_t n,
                              uint32_t window,
                              uint8_t* out, const uint64_t* out_off,
                              uint64_t* out_bytes, int32_t* err);
SQZ_API int sqz_decode_blocks(const uint8_t* in, const uint64_t* in_off, uint32_t n,
                              uint8_t* out, const uint64_t* out_off,
                              int32_t* err);

/* Device-resident flavour: every pointer is a DEVICE pointer on the current
 * HIP device (hipMalloc / torch.cuda tensor storage), `stream` is a
 * hipStream_t (NULL = default stream).  Asynchronous: returns after enqueue.
 * `scratch` must hold sqz_hip_encode_scratch_bytes(n, in_off[n]): the per-byte work arrays
 * are addressed by the ABSOLUTE offsets in d_in_off (in_off[0] need not be 0).  The offsets
 * live on the device, so a scratch that is too small cannot be told at the call: the kernels
 * refuse every block whose in_off[b+1] lies beyond it -- err[b] = EINVAL, out_bytes[b] = 0,
 * nothing written out of bounds -- and the other blocks are unaffected.                    */
SQZ_API uint64_t sqz_hip_encode_scratch_bytes(uint32_t n, uint64_t total_in_bytes);
SQZ_API int sqz_hip_encode_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                  uint32_t window,
                                  void* d_out, const uint64_t* d_out_off,
                                  uint64_t* d_out_bytes, int32_t* d_err,
                                  void* d_scratch, uint64_t scratch_bytes,
                                  void* stream);
SQZ_API uint64_t sqz_hip_decode_scratch_bytes(uint32_t n, uint64_t total_out_bytes);
SQZ_API int sqz_hip_decode_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                  void* d_out, const uint64_t* d_out_off,
                                  int32_t* d_err, void* d_scratch, uint64_t scratch_bytes,
                                  void* stream);

/* The two encode stages on their own (parity tests pin each independently,
 * SURVEY.md section 8c; also what a caller with its own entropy stage binds):
 *  stage 1  squeeze.h:338-358 + greedy step :377-394 -> token words
 *           literal 0x000000bb ; match 0x80000000 | len<<16 | dist
 *           block b's tokens start at d_tokens + in_off[b] (one slot per byte)
 *  stage 2  squeeze.h:278-315 + huffman.h + bitstream.h -> payload bytes    */
SQZ_API int sqz_hip_lz77_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                uint32_t window, uint32_t* d_tokens,
                                uint32_t* d_token_count, void* stream);
/* stage 1 with an explicit match finder: 0 = brute-force scan (squeeze.h:340-358 as
 * written), 1 = indexed (same tokens; visits only the earlier positions that share
 * the 3-byte prefix, nearest first -- SURVEY.md section 8f-3).  finder 1 needs
 * d_work = 8 bytes per input byte (+512).                                        */
SQZ_API int sqz_hip_lz77_blocks_ex(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                   uint32_t window, uint32_t* d_tokens,
                                   uint32_t* d_token_count, int finder,
                                   void* d_work, uint64_t work_bytes, void* stream);
/* stage 2 alone, on the caller's token words.  Every word is checked (a byte, or len 3..257 and
 * dist 1..32767, no stray bits) and a block may not hold more tokens than it has slots: a
 * violation fails that block with err[b] = EINVAL, other blocks are unaffected.  Whether the
 * tokens describe a consistent text (distances within what precedes them, lengths adding up) is
 * the caller's business: an inconsistent sequence encodes to a stream the decoder rejects. */
SQZ_API int sqz_hip_huffman_blocks(const uint32_t* d_tokens, const uint64_t* d_in_off,
                                   const uint32_t* d_token_count, uint32_t n,
                                   void* d_out, const uint64_t* d_out_off,
                                   uint64_t* d_out_bytes, int32_t* d_err,
                                   void* stream);

/* Counters the reference keeps next to the hot path, per block, opt-in:
 *   huffman.h:29-33   stats.updates (huffman_update_paths calls, one per node visited, :42),
 *                     stats.swaps (:76), stats.moves (:111), for each tree
 *   squeeze.h:327-328,386,391  li_bytes / br_bytes: source bytes coded as literals / as back
 *                     references (what SQUEEZE_MAP_STATS prints as percentages, :397-403)
 *   huffman.h:26      the depth marks at the end;  huffman.h:237-249 huffman_entropy is
 *                     sqz_stats_entropy() over the leaf counts returned here
 * Pass a device array of n entries to sqz_hip_encode_blocks_stats (NULL = no counters).
 * The update counter follows the reference while a tree is shallower than 26 levels (any
 * stream of less than 2^25 symbols); deeper trees keep swaps / moves only.                  */
typedef struct sqz_block_stats {
    uint32_t lit_updates, lit_swaps, lit_moves;
    uint32_t pos_updates, pos_swaps, pos_moves;
    uint32_t literal_bytes, backref_bytes;
    uint32_t lit_depth, pos_depth;
    uint32_t tokens, reserved;
    uint32_t lit_freq[288];      /* count of every leaf of the literal/length tree (symbol = index) */
    uint32_t pos_freq[32];       /* ... of the distance tree */
} sqz_block_stats;
SQZ_API int sqz_hip_encode_blocks_stats(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                        uint32_t window,
                                        void* d_out, const uint64_t* d_out_off,
                                        uint64_t* d_out_bytes, int32_t* d_err,
                                        void* d_scratch, uint64_t scratch_bytes,
                                        sqz_block_stats* d_stats, void* stream);
/* huffman.h:237-249: Shannon entropy (bits per symbol) of `n` leaf counts.  Host arithmetic. */
SQZ_API double sqz_stats_entropy(const uint32_t* freq, uint32_t n);

/* Test entry: drive ONE adaptive Huffman tree on the device with a symbol sequence through
 * huffman_inc_frequency semantics (huffman.h:218-235; unseen symbol -> huffman_insert :149) --
 * exactly the code paths the encoder uses: runs of attached symbols in batches of `batch`
 * (1..64) through the batched update, everything else one at a time -- and dump its node arrays.
 * which: 0 = the literal/length tree (n = 512 in the reference, 288 leaf ids here), 1 = the
 * distance tree (n = 32).  d_dump: 8 + 4 * nodes uint32 (nodes = 576 / 64):
 *   [0..7]  next id, depth mark (huffman.h:26), complete (:27), intervals kept, fault,
 *           stats.updates, stats.swaps, stats.moves (huffman.h:29-33)
 *   then per node id v:  up | lo << 10 | hi << 20 (0x3FF = none; ids are absolute: + 576 for the
 *           distance tree),  st | en << 9 | partner << 18,  count | depth << 24,  code (leaves)
 * Leaves keep their symbol value as id, the root is id `leaves`, internal nodes count up from it
 * (the reference counts down from 2n-2; no emitted bit depends on the numbering).           */
SQZ_API int sqz_hip_debug_tree(const int32_t* d_symbols, uint32_t count, int which, int batch,
                               uint32_t* d_dump, void* stream);

/* Streams of a batch, back to back: stream b moves from d_slabs + d_slab_off[b] (where
 * sqz_hip_encode_blocks left it) to d_dense + d_dense_off[b]; d_dense_off = exclusive prefix
 * sum of d_bytes, every entry a multiple of 8 (n + 1 entries, computed by the caller on the device).  The dense image with
 * d_dense_off as offsets is what sqz_hip_decode_blocks reads, and what the multi-GPU gather
 * of SURVEY.md section 8e ships (110 MB per 512 blocks instead of 269 MB of slabs).
 * avg_bytes sizes the launch (total / n is fine).  All device pointers, asynchronous.       */
SQZ_API int sqz_hip_pack_blocks(const void* d_slabs, const uint64_t* d_slab_off,
                                const uint64_t* d_bytes, uint32_t n,
                                void* d_dense, const uint64_t* d_dense_off,
                                uint64_t avg_bytes, void* stream);

/* ------------------------------------------------------------------ */
/* SQZF: a checksummed, seekable frame around the block streams -- ONE artifact for one large
 * buffer, decodable without side information.  This is THIS PROJECT'S format, not the
 * reference's ("block size is part of the format the build defines"); the
 * streams inside are exactly what sqz_encode_blocks produces, bit-identical to the reference's
 * squeeze_compress output for each block without its 72-bit header.  Version 1, all integers
 * little-endian:
 *
 *   offset  size  field
 *   0       4     magic  53 51 5A 46  ("SQZF")
 *   4       1     version = 1
 *   5       1     win_bits      10..15  (window = 1 << win_bits for every block)
 *   6       1     block_bits    12..24  (block_bytes = 1 << block_bits)
 *   7       1     flags = 0     (a reader refuses any other value)
 *   8       8     content_bytes           uncompressed length
 *   16      8     payload_bytes           sum of all stream lengths
 *   24      4     n_blocks = ceil(content_bytes / block_bytes)   (0 for empty content)
 *   28      4     index_crc     CRC-32 over bytes [0,28) followed by the whole index
 *   32      8*n   index: per block { u32 stream_words ; u32 content_crc }
 *   ..            zero padding to the next multiple of 16  -> payload_off
 *   payload_off   the n streams back to back, stream b is stream_words[b] * 8 bytes
 *
 * Block b covers content bytes [b * block_bytes, min((b+1) * block_bytes, content_bytes)).
 * content_crc is the CRC-32 of the block's uncompressed bytes as zlib's crc32 computes it (IEEE
 * 802.3, reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF); index_crc is
 * the same function.  frame_bytes = payload_off + payload_bytes: 32 for empty content.
 *
 * Errors: EINVAL a malformed header or argument, EILSEQ a checksum that does not match, E2BIG
 * a buffer (avail, capacity) that is too small.
 *
 * Version 2 = version 1 with stored blocks: content that does not compress is carried as it is.
 * Header, index entries, payload_off and both checksums keep their place and meaning; what differs:
 *
 *   4       1     version = 2
 *   7       1     flags = SQZ_FRAME_STORED (bit 0).  A version-2 header always has a non-zero flags
 *                 whose bits are all known: version 2 with flags 0 or with any of bits 1..7, and
 *                 version 1 with any flag, are EINVAL.  A frame that uses no feature is version 1.
 *   16      8     payload_bytes = sum of payload_words * 8 over all blocks, stored or not
 *   32      8*n   index: per block { u32 payload_words | stored << 31 ; u32 content_crc }
 *
 * payload_words * 8 is the block's share of the payload (a stream is at most 2 * 2^24 + 1024 bytes,
 * so bit 31 is free).  A stored block's share is its content followed by zeros up to the next
 * multiple of 8: payload_words == ceil(length / 8) exactly, anything else is EINVAL; readers do not
 * look at the padding.  content_crc covers the content and is verified for stored blocks too.
 * Writer's rule, exact, so that any writer reproduces a frame byte for byte: block b is stored iff
 * stream_bytes(b) >= length(b) -- streams are multiples of 8, so iff the stored form is not larger.
 * A writer asked for SQZ_FRAME_STORED writes version 2 whether or not a block ends up stored: one
 * byte of content is a stored block (8 >= 1), empty content a 32-byte version-2 header.  Worst case:
 * frame_bytes <= pad16(32 + 8n) + round_up_8(content_bytes).                                 */
enum {
    sqz_frame_header_bytes   = 32,
    sqz_frame_min_block_bits = 12,
    sqz_frame_max_block_bits = 24
};
enum { SQZ_FRAME_STORED = 1,     /* flags: store a block raw when its stream is not smaller (version 2) */
       SQZ_FRAME_DICT = 2,       /* flags: every block may reach back into one shared dictionary (version 3, below) */
       SQZ_FRAME_SHUFFLE = 4 };  /* flags: every block is byte-shuffled in front of the encoder (version 4, below) */
struct sqz_frame_info {
    uint64_t content_bytes, payload_bytes, payload_off, frame_bytes, block_bytes;
    uint32_t n_blocks, win_bits, version, reserved;     /* reserved: the header's flags */
};
/* one block of a frame: where its share of the payload lies (payload_off from the start of the
 * frame), what it decodes to, and whether it is stored */
struct sqz_frame_block {
    uint64_t payload_off, payload_bytes, content_bytes;
    uint32_t content_crc, stored;
};

/* Host code, no device is touched (like sqz_file_words). */
/* worst-case frame_bytes: header + index + padding + sqz_bound per block; 0 for a block_bits
 * outside 12..24 */
SQZ_API uint64_t sqz_frame_bound(uint64_t content_bytes, uint32_t block_bits);
/* the same for a frame written with `flags`: sqz_frame_bound for 0; for SQZ_FRAME_STORED
 * pad16(32 + 8n) + round_up_8(content_bytes); 0 for any other flags (a version-3 frame: sqz_frame_bound_dict) */
SQZ_API uint64_t sqz_frame_bound_ex(uint64_t content_bytes, uint32_t block_bits, uint32_t flags);
/* Parses and checks the header from the first `avail` bytes (E2BIG when avail < 32): magic,
 * version, flags, the ranges of win_bits / block_bits, n_blocks == ceil(content_bytes /
 * block_bytes), no overflow in 32 + 8n or frame_bytes (EINVAL).  When avail also covers the
 * index: index_crc (EILSEQ), and that the stream_words sum to payload_bytes / 8 (EINVAL).   */
SQZ_API int sqz_frame_info(const uint8_t* frame, uint64_t avail, struct sqz_frame_info* out);
/* Blocks [first, first + count) of a frame of either version, whose header, index and padding up to
 * payload_off lie inside avail (E2BIG otherwise; every check of sqz_frame_info applies): what a
 * caller needs to fetch one block's bytes from storage.  EINVAL when the range leaves the frame. */
SQZ_API int sqz_frame_blocks(const uint8_t* frame, uint64_t avail, uint32_t first, uint32_t count,
                             struct sqz_frame_block* out);

/* Host buffers in, host buffers out (H2D + kernels + D2H inside, on a leased lane's stream).
 * The encode scratch is 8 bytes per input byte, so both directions work through the buffer in
 * PASSES of whole blocks, at most 1 GiB of content each (SQZ_FRAME_PASS_BYTES overrides; one
 * block at least), and still produce / consume one frame.
 * compress: E2BIG when `capacity` is too small; *frame_bytes is the size needed either way and
 *   nothing is written beyond capacity.
 * decompress: accepts avail >= frame_bytes (a frame may be followed by another record).
 *   Returns 0 only when every block decoded and every checksum matched.  block_err (optional,
 *   n_blocks entries): a block whose stream the decoder rejects keeps the decoder's errno, one
 *   that decodes to the wrong bytes gets EILSEQ; the call returns the first non-zero one.  Good
 *   blocks are still delivered.  E2BIG when capacity < content_bytes or avail < frame_bytes.
 * read: content bytes [offset, offset + length) -> out.  Uploads and decodes only the covering
 *   blocks (plus header and index), verifies their checksums, copies back only the range.
 *   EINVAL when the range leaves the content.                                               */
SQZ_API int sqz_frame_compress(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                               uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes);
/* compress_ex: flags = 0 is sqz_frame_compress; SQZ_FRAME_STORED writes version 2 (every block is still
 * encoded: the rule needs its stream's size); other flags EINVAL.  Readers take both versions.  */
SQZ_API int sqz_frame_compress_ex(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                                  uint32_t flags, uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes);
SQZ_API int sqz_frame_decompress(const uint8_t* frame, uint64_t avail, uint8_t* data, uint64_t capacity,
                                 uint64_t* bytes, int32_t* block_err);
SQZ_API int sqz_frame_read(const uint8_t* frame, uint64_t avail, uint64_t offset, uint64_t length,
                           uint8_t* out);

/* Device-resident flavour: every pointer a DEVICE pointer (d_frame 16-byte aligned), asynchronous,
 * no host synchronisation inside.  The stream sizes are only known on the device, so the prefix
 * sum, the index, payload_bytes, index_crc and the compaction of the slabs all happen in kernels.
 * encode: *d_frame_bytes (u64) = the size needed; *d_status (i32) = 0, E2BIG when that exceeds
 *   `capacity` (nothing is written to d_frame then), or the first failed block's errno; d_err has
 *   n_blocks = ceil(content_bytes >> block_bits) entries.
 * decode: n_blocks and content_bytes are what sqz_frame_info said about a host copy of the 32
 *   header bytes; avail must cover header and index (E2BIG at the call otherwise).  A kernel checks
 *   that the device header agrees, index_crc, the stream_words sum and that the payload lies inside
 *   avail.  If any of that fails *d_status is set (EINVAL / EILSEQ / E2BIG), every d_err[b] gets
 *   the same value and no kernel reads the payload or writes d_out: a corrupt frame is refused by
 *   arithmetic.  Otherwise d_err[b] as for sqz_frame_decompress.  d_out holds content_bytes.    */
SQZ_API uint64_t sqz_hip_frame_scratch_bytes(uint64_t content_bytes, uint32_t block_bits, int encode);
SQZ_API int sqz_hip_frame_encode(const void* d_in, uint64_t content_bytes, uint32_t win_bits,
                                 uint32_t block_bits, void* d_frame, uint64_t capacity,
                                 uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err,
                                 void* d_scratch, uint64_t scratch_bytes, void* stream);
/* the _ex calls: flags as for sqz_frame_compress_ex.  A version-2 encode needs the scratch of
 * sqz_hip_frame_scratch_bytes_ex(.., 1, SQZ_FRAME_STORED) (a mask more than version 1); a decode of
 * either version needs what sqz_hip_frame_scratch_bytes(.., 0) says.  The frames equal the host
 * flavour's byte for byte; a version-2 frame always fits sqz_frame_bound_ex bytes.
 * sqz_hip_frame_decode cannot know the version without a host copy of the header, so it decodes
 * every frame, version 1 included, with the mask-aware decode kernels and one launch of the copy
 * kernel (all of whose workgroups leave at once for a version-1 frame): same results, but not the
 * machine code that decoded a version-1 frame before.  The host calls know the version and decode
 * a version-1 frame exactly as before.                                                         */
SQZ_API uint64_t sqz_hip_frame_scratch_bytes_ex(uint64_t content_bytes, uint32_t block_bits, int encode,
                                                uint32_t flags);
SQZ_API int sqz_hip_frame_encode_ex(const void* d_in, uint64_t content_bytes, uint32_t win_bits,
                                    uint32_t block_bits, uint32_t flags, void* d_frame, uint64_t capacity,
                                    uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err,
                                    void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_frame_decode(const void* d_frame, uint64_t avail, uint32_t n_blocks,
                                 uint64_t content_bytes, void* d_out, int32_t* d_err, int32_t* d_status,
                                 void* d_scratch, uint64_t scratch_bytes, void* stream);
/* The checksum kernel on its own: d_crc[b] = CRC-32 (zlib) of d_in[d_in_off[b] .. d_in_off[b+1]),
 * n ragged ranges at arbitrary (unaligned) offsets; n + 1 offsets, n results.               */
SQZ_API int sqz_hip_crc32_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                 uint32_t* d_crc, void* stream);

/* which finder sqz_compress / sqz_*encode_blocks use: 1 = indexed (default),
 * 0 = brute-force scan; also settable with SQZ_FINDER=scan|index.           */
SQZ_API void sqz_hip_set_finder(int finder);
SQZ_API int  sqz_hip_get_finder(void);

/* The parse as a per-call argument.  SQZ_PARSE_GREEDY is the reference's step (squeeze.h:377-394): through a
 * _parse call it is the call without the suffix, the same kernels and the same bytes.  SQZ_PARSE_LAZY looks one
 * position ahead: with L(i) the longest match at i (the finder's: strict >, nearest first, 0 or 3..257),
 *     L(i) >= 3, i + 1 < n and L(i + 1) > L(i)   ->  the literal data[i], on to i + 1
 *     otherwise L(i) >= 3                         ->  the match at i, on to i + L(i)
 *     otherwise                                   ->  the literal data[i], on to i + 1
 * No thresholds; one position after the other may give way.  The streams are NOT the reference's streams, but
 * they are streams of the same format: every decoder here and the reference's own read them.  2-4 % smaller on
 * text and executables, now and then larger (0.6 % on a bitmap): opt-in.  The lazy parse reads the match table
 * and therefore always runs the indexed finder, whatever sqz_hip_set_finder / SQZ_FINDER say;
 * sqz_hip_lz77_blocks_parse with finder 0 and SQZ_PARSE_LAZY is EINVAL.  Any other parse value is EINVAL at the
 * call: nothing is launched, nothing written.  Every call is its counterpart plus `parse`: same arguments, same
 * scratch sizes, same errors (ENODEV without a device).  The parse is not recorded in a frame: a lazy frame is an
 * ordinary version-1 frame, or version 2 with SQZ_FRAME_STORED, whose rule then looks at the lazy stream's size. */
#define SQZ_PARSE_GREEDY 0u
#define SQZ_PARSE_LAZY 1u
SQZ_API int sqz_encode_blocks_parse(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint32_t window,
                                    uint32_t parse, uint8_t* out, const uint64_t* out_off,
                                    uint64_t* out_bytes, int32_t* err);
SQZ_API int sqz_hip_encode_blocks_parse(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                                        uint32_t parse, void* d_out, const uint64_t* d_out_off,
                                        uint64_t* d_out_bytes, int32_t* d_err,
                                        void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_lz77_blocks_parse(const void* d_in, const uint64_t* d_in_off, uint32_t n,
                                      uint32_t window, uint32_t* d_tokens,
                                      uint32_t* d_token_count, int finder, uint32_t parse,
                                      void* d_work, uint64_t work_bytes, void* stream);
SQZ_API int sqz_frame_compress_parse(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                                     uint32_t flags, uint32_t parse, uint8_t* frame, uint64_t capacity,
                                     uint64_t* frame_bytes);
SQZ_API int sqz_hip_frame_encode_parse(const void* d_in, uint64_t content_bytes, uint32_t win_bits,
                                       uint32_t block_bits, uint32_t flags, uint32_t parse, void* d_frame,
                                       uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status,
                                       int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* A shared dictionary: frames of SMALL blocks that still compress.  A ranged read pays off with small blocks (a
 * block is one wave's dependent chain), and small blocks compress badly: each starts with empty trees and an empty
 * window.  The caller supplies one dictionary of 1 .. window - 1 bytes, and every block may reach back into it as
 * if it stood directly in front of the block: the stream of block B under dictionary Dct is exactly what the
 * reference's encoder writes for the bytes Dct || B when it starts, with fresh trees, at position D = len(Dct).
 * At block position i the candidates are the distances 1 .. min(D + i, window - 1), nearest first, a candidate
 * replaces the best only when strictly longer, lengths count up to min(len(B) - i, 257), and a source may begin in
 * the dictionary and run on into the block.  Tokens, entropy stage and stream format are unchanged (a distance is
 * still at most 0x7FFF); blocks stay independent of each other.  The caller keeps the dictionary: it is not
 * carried in the stream or the frame.  Opt-in like the lazy parse, and for the same reason: text gains 10-25 % at
 * 1-16 KB blocks, an executable with its own header as dictionary LOSES 6 % (the greedy rule takes every 3-byte
 * match, however far away).  The caller chooses the dictionary.
 *
 * Every call is its counterpart plus `dict, dict_bytes` (the encode calls also take `parse`), with the same
 * errors otherwise.  dict == NULL, dict_bytes == 0 and dict_bytes > window - 1 (decode calls, which have no
 * window: > 32767) are EINVAL at the call: nothing is launched.  The scan finder has no match table to merge the
 * dictionary's matches into: sqz_hip_lz77_blocks_dict with finder 0 is EINVAL, and the encode calls run the
 * indexed finder whatever sqz_hip_set_finder says.  Device flavour: d_dict is a device pointer.  The encode
 * scratch grows by the dictionary's index, built once per call by index_sort_kernel:
 *     sqz_hip_encode_scratch_bytes_dict(n, total, D) = sqz_hip_encode_scratch_bytes(n, total)
 *                                                      + 256 + 2 * round_up_256(4 * (D + 64))      (<= 262,912)
 * and sqz_hip_lz77_blocks_dict's d_work by the same amount (d_work and d_scratch 16-byte aligned).  A decode
 * needs the scratch of sqz_hip_decode_blocks.  The decoder refuses a distance that reaches in front of the
 * dictionary (dist > position + dict_bytes) with EINVAL for that block, as it refuses dist > position without.  */
SQZ_API int sqz_encode_blocks_dict(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint32_t window,
                                   uint32_t parse, const uint8_t* dict, uint64_t dict_bytes, uint8_t* out,
                                   const uint64_t* out_off, uint64_t* out_bytes, int32_t* err);
SQZ_API int sqz_decode_blocks_dict(const uint8_t* in, const uint64_t* in_off, uint32_t n, const uint8_t* dict,
                                   uint64_t dict_bytes, uint8_t* out, const uint64_t* out_off, int32_t* err);
SQZ_API uint64_t sqz_hip_encode_scratch_bytes_dict(uint32_t n, uint64_t total_in_bytes, uint64_t dict_bytes);
SQZ_API int sqz_hip_encode_blocks_dict(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                                       uint32_t parse, const void* d_dict, uint64_t dict_bytes, void* d_out,
                                       const uint64_t* d_out_off, uint64_t* d_out_bytes, int32_t* d_err,
                                       void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_decode_blocks_dict(const void* d_in, const uint64_t* d_in_off, uint32_t n, const void* d_dict,
                                       uint64_t dict_bytes, void* d_out, const uint64_t* d_out_off, int32_t* d_err,
                                       void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_lz77_blocks_dict(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                                     uint32_t* d_tokens, uint32_t* d_token_count, int finder, uint32_t parse,
                                     const void* d_dict, uint64_t dict_bytes, void* d_work, uint64_t work_bytes,
                                     void* stream);

/* SQZF version 3 = version 2's layout with flags bit 1 (SQZ_FRAME_DICT) and one 8-byte record directly behind the
 * n index entries:
 *
 *   4         1   version = 3.  A header is version 3 iff bit 1 of flags is set: version 3 without it or with any
 *                 of bits 2..7, and version 1 or 2 with bit 1, are EINVAL.  Bit 0 (SQZ_FRAME_STORED) may accompany
 *                 it with its unchanged rule, stored iff stream_bytes(b) >= length(b); a stored block ignores the
 *                 dictionary, and a stored entry in a frame without bit 0 is EINVAL.
 *   32 + 8n   4   dict_bytes    1 .. window - 1 (anything else EINVAL)
 *   36 + 8n   4   dict_crc      CRC-32 (zlib) of the dictionary
 *   ..            zero padding to the next multiple of 16 -> payload_off = pad16(32 + 8n + 8)
 *
 * index_crc covers bytes [0,28), the index and the record.  A frame written without a dictionary is byte for
 * byte what it always was.  sqz_frame_info and sqz_frame_blocks accept version 3 (struct sqz_frame_info is
 * unchanged: version = 3, reserved = flags); sqz_frame_dict reads the record (EINVAL for versions 1 and 2, E2BIG
 * when avail does not cover it); sqz_frame_bound_dict is the worst case of a frame written by
 * sqz_frame_compress_dict with the same flags (sqz_frame_bound_ex's with the record's 8 bytes in front of the
 * padding; sqz_frame_bound_ex itself keeps answering 0 for any flag but SQZ_FRAME_STORED).
 * Host flavour only.  compress_dict: flags 0 or SQZ_FRAME_STORED, with or without SQZ_FRAME_DICT, which is set in
 * the header either way.  The dictionary is uploaded and indexed once per call, not once per pass.  A _dict
 * reader first compares dict_bytes and the CRC-32 of the dictionary it was given with the record: a mismatch is
 * EILSEQ for the call and for every block (block_err), nothing is decoded and nothing is written; a frame of
 * version 1 or 2 is EINVAL.  sqz_frame_decompress and sqz_frame_read answer EINVAL for a version-3 frame.
 * The device-resident calls above keep to versions 1 and 2: sqz_hip_frame_encode* with SQZ_FRAME_DICT are EINVAL,
 * sqz_hip_frame_scratch_bytes_ex answers 0 for it, and sqz_hip_frame_decode refuses a version-3 frame by arithmetic
 * (*d_status = EINVAL, nothing decoded).  Version 3 on the device has calls of its own, further down:
 * sqz_hip_frame_encode_dict, sqz_hip_frame_decode_dict, sqz_hip_frame_read_dict.                             */
SQZ_API int sqz_frame_dict(const uint8_t* frame, uint64_t avail, uint32_t* dict_bytes, uint32_t* dict_crc);
SQZ_API uint64_t sqz_frame_bound_dict(uint64_t content_bytes, uint32_t block_bits, uint32_t flags);
SQZ_API int sqz_frame_compress_dict(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                                    uint32_t flags, uint32_t parse, const uint8_t* dict, uint64_t dict_bytes,
                                    uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes);
SQZ_API int sqz_frame_decompress_dict(const uint8_t* frame, uint64_t avail, const uint8_t* dict, uint64_t dict_bytes,
                                      uint8_t* data, uint64_t capacity, uint64_t* bytes, int32_t* block_err);
SQZ_API int sqz_frame_read_dict(const uint8_t* frame, uint64_t avail, const uint8_t* dict, uint64_t dict_bytes,
                                uint64_t offset, uint64_t length, uint8_t* out);

/* SQZF version 4 = version 2's layout with flags bit 2 (SQZ_FRAME_SHUFFLE) and one 8-byte record directly behind the
 * n index entries, the place and shape of version 3's:
 *
 *   4         1   version = 4.  A header is version 4 iff bit 2 of flags is set: version 4 without it or with any
 *                 of bits 3..7, and versions 1 to 3 with bit 2, are EINVAL; so is bit 1 (SQZ_FRAME_DICT) together with
 *                 bit 2, everywhere.  Bit 0 (SQZ_FRAME_STORED) may accompany it; a stored entry in a frame without
 *                 bit 0 is EINVAL.
 *   32 + 8n   4   elem_bytes    2, 4 or 8 (anything else EINVAL)
 *   36 + 8n   4   zero          (anything else EINVAL)
 *   ..            zero padding to the next multiple of 16 -> payload_off = pad16(32 + 8n + 8)
 *
 * index_crc covers bytes [0,28), the index and the record; the record's fields and the stored entries are looked at
 * only once it has held.  With B a block of L bytes, e = elem_bytes and m = L / e rounded down, the block's stream is
 * exactly the encoder's stream (greedy or lazy parse) for S, where
 *     S[j * m + i] = B[i * e + j]    0 <= i < m, 0 <= j < e
 * and the L - m * e tail bytes keep their place behind the planes.  content_crc is over B, the caller's bytes.  The
 * stored rule is unchanged and exact, stored iff stream_bytes(S) >= L, and a stored block carries B, not S.  Blocks
 * stay independent: ranged reads work as ever.  Empty content is a 48-byte frame.  A frame written without the
 * filter is byte for byte what it always was.
 * sqz_frame_info and sqz_frame_blocks accept version 4 (struct sqz_frame_info is unchanged: version = 4, reserved =
 * flags); sqz_frame_elem reads the record (EINVAL for versions 1 to 3, E2BIG when avail does not cover it);
 * sqz_frame_bound_shuf is the worst case of a frame written by sqz_frame_compress_shuf with the same flags
 * (sqz_frame_bound_ex's for flags & SQZ_FRAME_STORED with the record's 8 bytes in front of the padding; 0 for any
 * flag but SQZ_FRAME_STORED and SQZ_FRAME_SHUFFLE; sqz_frame_bound_ex and sqz_frame_bound_dict keep answering 0 for
 * SQZ_FRAME_SHUFFLE).
 * compress_shuf: flags 0 or SQZ_FRAME_STORED, with or without SQZ_FRAME_SHUFFLE, which is set in the header either
 * way; EINVAL for any other flag (SQZ_FRAME_DICT among them), elem_bytes other than 2, 4, 8, a parse that is none.  It
 * works in sqz_frame_compress's passes of whole blocks; a pass lies on the device once more, shuffled.
 * decompress_shuf / read_shuf: sqz_frame_decompress / sqz_frame_read for frames of versions 1, 2 and 4 (EINVAL for
 * version 3); the decoder's output of a pass lies in the scratch and the inverse shuffle writes the blocks that are
 * not stored.  Every call there was keeps refusing a version-4 frame with EINVAL: sqz_frame_decompress,
 * sqz_frame_read, the _dict readers, sqz_hip_frame_decode, sqz_hip_frame_read, and gather, update and append in both
 * flavours (those three on version 4 are a later step).                                                          */
SQZ_API int sqz_frame_elem(const uint8_t* frame, uint64_t avail, uint32_t* elem_bytes);
SQZ_API uint64_t sqz_frame_bound_shuf(uint64_t content_bytes, uint32_t block_bits, uint32_t flags);
SQZ_API int sqz_frame_compress_shuf(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                                    uint32_t flags, uint32_t parse, uint32_t elem_bytes, uint8_t* frame,
                                    uint64_t capacity, uint64_t* frame_bytes);
SQZ_API int sqz_frame_decompress_shuf(const uint8_t* frame, uint64_t avail, uint8_t* data, uint64_t capacity,
                                      uint64_t* bytes, int32_t* block_err);
SQZ_API int sqz_frame_read_shuf(const uint8_t* frame, uint64_t avail, uint64_t offset, uint64_t length, uint8_t* out);

/* The byte shuffle on its own: n ragged ranges, range b = [d_off[b], d_off[b + 1]) of d_in and of d_out alike (d_off:
 * n + 1 offsets in DEVICE memory), each transposed on its own as above (inverse != 0: back).  Any alignment of the
 * pointers and offsets; d_in and d_out must not overlap; nothing outside a range is read or written.  Asynchronous
 * on `stream`.  EINVAL: elem_bytes other than 2, 4, 8, a null pointer with n > 0, d_in == d_out.  Not among the
 * kernels of sqz_hip_timing.                                                                                     */
SQZ_API int sqz_hip_shuffle_blocks(const void* d_in, const uint64_t* d_off, uint32_t n, uint32_t elem_bytes,
                                   int inverse, void* d_out, void* stream);

/* Version 4 in the device-resident flavour.  Every pointer a DEVICE pointer (d_frame and d_scratch 16-byte aligned),
 * asynchronous, no host synchronisation inside; d_frame_bytes, d_status, d_err as for the _dict calls below.
 * Call-level EINVAL, before the device is touched: elem_bytes other than 2, 4, 8, a parse that is none, flags other
 * than SQZ_FRAME_STORED and SQZ_FRAME_SHUFFLE, null or misaligned d_frame / d_scratch, a scratch smaller than the
 * formula says.  Every refusal leaves the output untouched.
 *
 * encode_shuf: the content is shuffled into the scratch and goes through the block encoder from there; checksums
 *   and stored blocks are taken from d_in.  The frame equals sqz_frame_compress_shuf's byte for byte and fits
 *   sqz_frame_bound_shuf.  Scratch:
 *       sqz_hip_frame_scratch_bytes_shuf(c, b, 1, flags) = sqz_hip_frame_scratch_bytes_ex(c, b, 1, flags & SQZ_FRAME_STORED)
 *                                                          + round_up_256(c + 16)
 *       sqz_hip_frame_scratch_bytes_shuf(c, b, 0, flags) = sqz_hip_frame_scratch_bytes(c, b, 0) + round_up_256(c + 16)
 *   and 0 for a block_bits outside 12..24 or any other flag.
 * decode_shuf: elem_bytes is what sqz_frame_elem said about a host copy of header, index and record; avail must
 *   cover them, 32 + 8 n + 8 bytes (E2BIG at the call otherwise).  A kernel checks, in this order: magic, version 4
 *   with flags bit 2 and none of bits 1, 3..7, field ranges (EINVAL; so a frame of versions 1 to 3 is EINVAL here);
 *   the header against n_blocks and content_bytes (EINVAL); index_crc over [0,28), index and record (EILSEQ); the
 *   record { 2 | 4 | 8, 0 } with the caller's elem_bytes (EINVAL); stored entries only with bit 0 and of their block's
 *   size (EINVAL); the words' sum against payload_bytes (EINVAL); the payload inside avail (E2BIG).  On any of these
 *   *d_status and every d_err[b] get that value and d_out is not written.  Otherwise the decoder writes into the
 *   scratch, the inverse shuffle writes the blocks that are not stored into d_out, the stored ones are copied, and
 *   checksums and d_err[b] are those of sqz_hip_frame_decode, over d_out.
 * read_shuf: sqz_hip_frame_read for a version-4 frame, with elem_bytes as for decode_shuf.  Scratch:
 *       sqz_hip_frame_read_scratch_bytes_shuf(length, b) = sqz_hip_frame_read_scratch_bytes(length, b)
 *                                                          + round_up_256((k << b) + 16)
 *       with k as there; 0 for a bad block_bits.                                                                 */
SQZ_API uint64_t sqz_hip_frame_scratch_bytes_shuf(uint64_t content_bytes, uint32_t block_bits, int encode, uint32_t flags);
SQZ_API int sqz_hip_frame_encode_shuf(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                                      uint32_t flags, uint32_t parse, uint32_t elem_bytes, void* d_frame,
                                      uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err,
                                      void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_frame_decode_shuf(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                      uint32_t elem_bytes, void* d_out, int32_t* d_err, int32_t* d_status,
                                      void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API uint64_t sqz_hip_frame_read_scratch_bytes_shuf(uint64_t length, uint32_t block_bits);
SQZ_API int sqz_hip_frame_read_shuf(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                    uint32_t block_bits, uint32_t elem_bytes, uint64_t offset, uint64_t length,
                                    void* d_out, int32_t* d_err, int32_t* d_status, void* d_scratch,
                                    uint64_t scratch_bytes, void* stream);

/* Version 3 in the device-resident flavour, and ranged reads from a frame that is already in device memory.  Every
 * pointer a DEVICE pointer (d_frame and d_scratch 16-byte aligned), asynchronous, no host synchronisation inside;
 * d_frame_bytes, d_status, d_err as for sqz_hip_frame_encode / sqz_hip_frame_decode.  Call-level EINVAL, before the
 * device is touched: d_dict == NULL, dict_bytes == 0, dict_bytes > window - 1 (encode) or > 32767 (decode, read), a
 * parse that is none, flags other than SQZ_FRAME_STORED and SQZ_FRAME_DICT, misaligned d_frame / d_scratch.
 *
 * encode_dict: flags 0 or SQZ_FRAME_STORED, with or without SQZ_FRAME_DICT, which is set in the header either way
 *   (sqz_frame_compress_dict's rule).  Always the indexed finder.  The dictionary is sorted once per call in the
 *   scratch, and its CRC-32 for the record is computed on the device.  The frame equals sqz_frame_compress_dict's
 *   byte for byte and fits sqz_frame_bound_dict.  Scratch:
 *       sqz_hip_frame_scratch_bytes_dict(c, b, 1, flags, D) = sqz_hip_frame_scratch_bytes_ex(c, b, 1, flags & SQZ_FRAME_STORED)
 *                                                             + 256 + 2 * round_up_256(4 * (D + 64))
 *       sqz_hip_frame_scratch_bytes_dict(c, b, 0, flags, D) = sqz_hip_frame_scratch_bytes(c, b, 0)
 *   and 0 for a block_bits outside 12..24, any other flag, or D outside 1..32767.
 * decode_dict: avail must cover header, index and record, 32 + 8 n + 8 bytes (E2BIG at the call otherwise).  A kernel
 *   checks, in this order: magic, version 3 with flags bit 1 and none of bits 2..7, field ranges (EINVAL; so a
 *   frame of version 1 or 2 is EINVAL here); the header against n_blocks and content_bytes (EINVAL); index_crc over
 *   [0,28), index and record (EILSEQ); the record's dict_bytes in 1 .. window - 1 (EINVAL); stored entries only with
 *   bit 0 and of their block's size (EINVAL); the words' sum against payload_bytes (EINVAL); the record against
 *   dict_bytes and the CRC-32 of d_dict, computed by a kernel just before (EILSEQ); the payload inside avail (E2BIG).
 *   On any of these *d_status and every d_err[b] get that value and d_out is not written: a wrong dictionary
 *   decodes nothing.  Otherwise d_err[b] as for sqz_frame_decompress_dict.
 * read / read_dict: content[offset, offset + length) of a resident frame of versions 1 and 2 / of version 3 into
 *   d_out.  n_blocks, content_bytes and block_bits are what sqz_frame_info said about a host copy of the 32 header
 *   bytes; the host works out the covering blocks, first = offset >> block_bits, from them.  EINVAL at the call: the
 *   range leaves the content, block_bits outside 12..24, n_blocks != ceil(content_bytes / 2^block_bits).  The
 *   covering blocks are decoded into the scratch and verified, d_err has ONE ENTRY PER COVERING BLOCK, and
 *   *d_status = the frame's status (the checks of sqz_hip_frame_decode / _decode_dict; EINVAL also for a frame whose
 *   block_bits is another), otherwise the first non-zero d_err.  d_out receives exactly `length` bytes when
 *   *d_status == 0 and is not written otherwise: a covering block that fails its decode or its checksum delivers
 *   nothing; a damaged block outside the range does not matter.  length == 0 sets *d_status = 0 on the stream and
 *   launches nothing else.  As for the decode calls the WHOLE frame, not only the covering streams, must lie inside
 *   avail (E2BIG in *d_status otherwise).  Scratch, the same for both calls, the worst case over every offset:
 *       sqz_hip_frame_read_scratch_bytes(length, b) = sqz_hip_frame_scratch_bytes(k << b, b, 0)
 *                                                     + round_up_256((k << b) + 16) + 256
 *       with k = ((length + 2^b - 2) >> b) + 1 covering blocks (k = 0 for length == 0); 0 for a bad block_bits.   */
SQZ_API uint64_t sqz_hip_frame_scratch_bytes_dict(uint64_t content_bytes, uint32_t block_bits, int encode,
                                                  uint32_t flags, uint64_t dict_bytes);
SQZ_API int sqz_hip_frame_encode_dict(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                                      uint32_t flags, uint32_t parse, const void* d_dict, uint64_t dict_bytes,
                                      void* d_frame, uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status,
                                      int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_frame_decode_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                      const void* d_dict, uint64_t dict_bytes, void* d_out, int32_t* d_err,
                                      int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API uint64_t sqz_hip_frame_read_scratch_bytes(uint64_t length, uint32_t block_bits);
SQZ_API int sqz_hip_frame_read(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                               uint32_t block_bits, uint64_t offset, uint64_t length, void* d_out, int32_t* d_err,
                               int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_frame_read_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                    uint32_t block_bits, uint64_t offset, uint64_t length, const void* d_dict,
                                    uint64_t dict_bytes, void* d_out, int32_t* d_err, int32_t* d_status,
                                    void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Many byte ranges of a resident frame in one call.  As sqz_hip_frame_read / _read_dict (device pointers, d_frame and
 * d_scratch 16-byte aligned, asynchronous, no host synchronisation inside; n_blocks, content_bytes and block_bits from
 * a host copy of the header), but d_offset and d_length, n_ranges values each, lie in DEVICE memory and are never read
 * by the host.  The host knows n_ranges, max_length -- a hard cap on every range's length -- and max_blocks, a cap on
 * the number of DISTINCT covering blocks (anything up to n_blocks; more counts as n_blocks;
 * min(n_blocks, n_ranges * (((max_length + 2^b - 2) >> b) + 1)) is always enough).
 *
 * Range r is valid iff length[r] <= max_length, offset[r] <= content_bytes and length[r] <= content_bytes - offset[r]
 * (no wrap of offset + length).  An invalid range gets d_range_err[r] = EINVAL, counts as length 0 and covers
 * nothing; a valid range of length 0 is delivered (0) and covers nothing.  d_out_off (n_ranges + 1 entries) is the
 * exclusive prefix sum of the valid ranges' lengths in request order: it depends on the ranges alone and is written
 * even when the frame is refused.  Range r is delivered to d_out[d_out_off[r], d_out_off[r + 1]).
 *
 * *d_status: the frame's status -- the checks of sqz_hip_frame_decode / _decode_dict in their order, EINVAL also for a
 *   frame whose block_bits is another, E2BIG unless the whole frame lies inside avail, EILSEQ for a wrong dictionary:
 *   *d_status and every valid range's d_range_err get it, *d_blocks_decoded = 0, d_out is not written.
 *   Otherwise ENOBUFS when the distinct covering blocks are more than max_blocks, else ENOSPC when
 *   d_out_off[n_ranges] > out_capacity: nothing is decoded, d_out is not written, every valid range's d_range_err gets
 *   the status, and *d_blocks_decoded still holds the distinct count, so the caller knows what to ask for.  Nothing is
 *   ever written past either cap.
 *   Otherwise 0: every distinct covering block is decoded ONCE into the scratch and verified against its CRC-32, and
 *   *d_blocks_decoded is their number.  For a valid range d_range_err[r] is the first non-zero errno among its
 *   covering blocks in ascending order (EILSEQ for a checksum that does not hold, otherwise the decoder's); a range
 *   with a non-zero value is NOT written, the others are: a damaged block costs the ranges that touch it and nothing
 *   else, and *d_status stays 0.
 * EINVAL at the call, nothing enqueued: block_bits outside 12..24; n_blocks != ceil(content_bytes / 2^block_bits); a
 *   null or misaligned d_frame / d_scratch; a null d_status, d_blocks_decoded or d_out_off; n_ranges > 0 with a null
 *   d_offset, d_length or d_range_err; max_blocks > 0 with a null d_out; a scratch smaller than the function says;
 *   _dict: d_dict == NULL or dict_bytes outside 1..32767.  E2BIG when avail does not cover header and index (and
 *   record), ENODEV without a device.  n_ranges == 0 writes d_out_off[0] = 0, *d_blocks_decoded = 0 and the frame's
 *   status and decodes nothing.
 * Scratch, with m = min(max_blocks, n_blocks), w = ceil(n_blocks / 32), every term rounded up to 256:
 *       sqz_hip_frame_gather_scratch_bytes(n_blocks, n_ranges, max_blocks, b) =
 *           2 * (4 w + 4) + 256 + (4 m + 4) + 2 * 8 (2 m + 1) + 4 * (8 m + 4) + (8 n_ranges + 8) + (4 n_ranges + 4)
 *           + sqz_hip_decode_scratch_bytes(2 m, m << b) + ((m << b) + 16)
 *   (bitmap and its prefix counts, control words, the list, two offsets per slot, four masks and results per slot, the
 *   copy's work list, the decoder's scratch, the decoded blocks); 0 for a bad block_bits.                            */
SQZ_API uint64_t sqz_hip_frame_gather_scratch_bytes(uint32_t n_blocks, uint32_t n_ranges, uint32_t max_blocks,
                                                    uint32_t block_bits);
SQZ_API int sqz_hip_frame_gather(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                 uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length,
                                 uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks, void* d_out,
                                 uint64_t out_capacity, uint64_t* d_out_off, int32_t* d_range_err,
                                 uint32_t* d_blocks_decoded, int32_t* d_status, void* d_scratch,
                                 uint64_t scratch_bytes, void* stream);
SQZ_API int sqz_hip_frame_gather_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                      uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length,
                                      uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks, const void* d_dict,
                                      uint64_t dict_bytes, void* d_out, uint64_t out_capacity, uint64_t* d_out_off,
                                      int32_t* d_range_err, uint32_t* d_blocks_decoded, int32_t* d_status,
                                      void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Many byte ranges WRITTEN into a resident frame in one call: the mirror of sqz_hip_frame_gather, and its conventions
 * (device pointers; d_frame, d_new_frame and d_scratch 16-byte aligned; asynchronous, no host synchronisation inside;
 * n_blocks, content_bytes, win_bits and block_bits from a host copy of the header -- win_bits because the encoder's
 * launches take the window from the host; d_offset and d_length in DEVICE memory, never read by the host; n_ranges,
 * max_length and max_blocks as for the gather, validity of a range by the gather's rule).  sqz_hip_frame_update is
 * for versions 1 and 2, _update_dict for version 3.
 *
 * d_data (data_bytes of it) holds the bytes to write, packed in request order; d_data_off (n_ranges + 1 entries) is
 * WRITTEN by the call: the exclusive prefix sum of the valid ranges' lengths.  It depends on the ranges alone and is
 * written even when the frame is refused, exactly like the gather's d_out_off.  Range r takes
 * d_data[d_data_off[r], d_data_off[r + 1]) to content[offset[r], offset[r] + length[r]).  Where two valid ranges overlap,
 * each overlapped byte takes the value of one of them, unspecified which (the rule of an indexed scatter); a block's
 * checksum is taken after the patch, so the frame is consistent either way.  parse: SQZ_PARSE_GREEDY or SQZ_PARSE_LAZY,
 * for the blocks that are encoded again.
 *
 * The new frame (d_new_frame, at most `capacity` bytes, *d_frame_bytes its size) keeps the old one's version, win_bits,
 * block_bits, flags, content_bytes and, in version 3, the dictionary's record: content length never changes.  Only the
 * DISTINCT covering blocks are touched: each is decoded into the scratch and verified against its CRC-32, patched,
 * checksummed again, encoded, and in a frame of version 2, or of version 3 with SQZ_FRAME_STORED, stored when its
 * stream is not smaller than its content (the writer's rule).  Every other block is KEPT: its index entry and its
 * stream are copied as they are, neither decoded nor verified -- a damaged kept block stays damaged and is still
 * reported by a later decode.  On status 0 the new frame is byte for byte what the encoder of that version writes for
 * the patched content with the same parse, provided the kept streams were written with that parse too.
 *
 * *d_status is the first of these that applies, and with ANY non-zero status not one byte of d_new_frame is written:
 *   1. the frame's own status: the checks of sqz_hip_frame_gather / _gather_dict in their order, then EINVAL for a
 *      frame whose win_bits is not the argument.  *d_blocks_encoded = 0.
 *   2. ERANGE: at least one range is invalid.  Those ranges have d_range_err[r] = EINVAL (every other one 0) and count
 *      as length 0 in d_data_off.  A write call does not silently drop a write: it refuses the lot.
 *   3. ENOBUFS: more distinct covering blocks than max_blocks.
 *   4. ENODATA: d_data_off[n_ranges] > data_bytes.
 *   5. the first non-zero errno among the touched blocks in ascending order: the decoder's, or EILSEQ for a checksum
 *      that does not hold.  The call does not build on content it cannot verify.
 *   6. a touched block's encoder errno (the first in ascending order).
 *   7. E2BIG: the new frame does not fit capacity; *d_frame_bytes is the size it takes.
 *   *d_frame_bytes is the frame's size for status 0 and for 7, and 0 for 1 to 6.  Under 1 to 4 nothing is decoded.
 *   *d_blocks_encoded is the number of distinct covering blocks of the valid ranges in every case but 1 (under 3: what
 *   to ask for).  A capacity of sqz_frame_bound / _bound_ex / _bound_dict for the frame's version is always enough.
 * n_ranges == 0 writes d_data_off[0] = 0 and a copy of the old frame (its exact bytes), or the frame's status.
 * EINVAL at the call, nothing enqueued: the gather's list (d_data_off for d_out_off, d_blocks_encoded for
 *   d_blocks_decoded; data_bytes > 0 with a null d_data for its d_out rule); win_bits outside 10..15; a null or
 *   misaligned d_new_frame; a null d_frame_bytes; [d_new_frame, + capacity) overlapping [d_frame, + avail) or the
 *   scratch; a parse that is none; a scratch smaller than the function says; _dict: d_dict == NULL or dict_bytes outside
 *   1 .. 2^win_bits - 1.  E2BIG when avail does not cover header and index (and record), ENODEV without a device.
 * Scratch, with m = min(max_blocks, n_blocks), w = ceil(n_blocks / 32), D = dict_bytes (0 for versions 1 and 2), every
 * term rounded up to 256:
 *       sqz_hip_frame_update_scratch_bytes(n_blocks, n_ranges, max_blocks, b, D) =
 *           2 * (4 w + 4) + 256 + (4 m + 4) + 2 * 8 (2 m + 1) + 4 * (8 m + 4) + (8 n_ranges + 8) + (4 n_ranges + 4)
 *           + ((m << b) + 16)                                         [so far the gather's terms without its decoder]
 *           + (8 n_ranges + 8) + 2 * 8 (m + 1) + (8 m + 8) + 2 * (4 m + 4)
 *           + 8 (2 m + 2) + 2 * 8 (2 m + 1) + 256 + (D > 0 ? 256 + 2 * round_up_256(4 * (D + 64)) : 0)
 *           + m * sqz_bound(2^b)
 *           + max(sqz_hip_decode_scratch_bytes(2 m, m << b), sqz_hip_encode_scratch_bytes(m, m << b))
 *   (the patch's destinations, the encoder's two offset lists, its sizes, errnos and the new checksums per slot, the
 *   three columns of the segment table, the verdict words, the dictionary's index, m slabs, and the encoder's scratch
 *   over the decoder's, which is done by then); 0 for a bad block_bits or D > 32767.                                   */
SQZ_API uint64_t sqz_hip_frame_update_scratch_bytes(uint32_t n_blocks, uint32_t n_ranges, uint32_t max_blocks,
                                                    uint32_t block_bits, uint64_t dict_bytes);
SQZ_API int sqz_hip_frame_update(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                 uint32_t win_bits, uint32_t block_bits, const uint64_t* d_offset,
                                 const uint64_t* d_length, uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks,
                                 const void* d_data, uint64_t data_bytes, uint64_t* d_data_off, uint32_t parse,
                                 void* d_new_frame, uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_range_err,
                                 uint32_t* d_blocks_encoded, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                                 void* stream);
SQZ_API int sqz_hip_frame_update_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                      uint32_t win_bits, uint32_t block_bits, const uint64_t* d_offset,
                                      const uint64_t* d_length, uint32_t n_ranges, uint64_t max_length,
                                      uint32_t max_blocks, const void* d_data, uint64_t data_bytes, uint64_t* d_data_off,
                                      uint32_t parse, const void* d_dict, uint64_t dict_bytes, void* d_new_frame,
                                      uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_range_err,
                                      uint32_t* d_blocks_encoded, int32_t* d_status, void* d_scratch,
                                      uint64_t scratch_bytes, void* stream);

/* More content BEHIND a resident frame in one call: the new frame is the frame of content || data.  The conventions
 * are the update's (device pointers; d_frame, d_new_frame and d_scratch 16-byte aligned; asynchronous, no host
 * synchronisation inside; n_blocks, content_bytes, win_bits and block_bits from a host copy of the header).
 * sqz_hip_frame_append is for versions 1 and 2, _append_dict for version 3.  There is no format change: the result is an
 * ordinary frame of the old one's version, and every reader takes it as it is.
 *
 * With C = content_bytes, A = data_bytes, b = block_bits: t = C mod 2^b is the number of bytes in a ragged last block,
 * keep = n_blocks - (t > 0 && A > 0 ? 1 : 0), m = ceil((t + A) / 2^b) for A > 0 (t counted only when t > 0) and 0 for
 * A == 0, and n' = keep + m.  The host knows all of these: no device count sizes a launch.
 *
 * The call writes a NEW frame into d_new_frame (at most `capacity` bytes, *d_frame_bytes its size); the old one is only
 * read and the two may not overlap.  The new frame keeps the old version, win_bits, block_bits and flags, and in
 * version 3 the dictionary's record; content_bytes = C + A, payload_bytes, n_blocks = n' and index_crc are new, and
 * payload_off is pad16(32 + 8 n' (+ 8)).  Blocks 0 .. keep - 1 are KEPT: their index entries and streams are copied as
 * they are, neither decoded nor verified -- a damaged kept block stays damaged and is still reported by a later
 * decode.  If t > 0 and A > 0 the old last block is TOUCHED: it is decoded into the head of a staging area in the
 * scratch (a stored block and a version-3 block with the dictionary as well) and verified against its CRC-32, and the
 * data follows it directly.  The m blocks of tail || data are checksummed, encoded (parse: SQZ_PARSE_GREEDY or
 * SQZ_PARSE_LAZY; with the dictionary in version 3) and, in a frame of version 2 or of version 3 with SQZ_FRAME_STORED,
 * stored when their stream is not smaller than their content (the writer's rule).  If t == 0 nothing is decoded.  On
 * status 0 the new frame is byte for byte what the encoder of that version writes for content || data with the same
 * parse, provided the kept streams were written with that parse too.
 * A == 0 writes a copy of the old frame (its exact bytes), or its status: nothing is decoded and nothing is encoded.
 * C == 0 is an empty frame (32 bytes, 48 with a dictionary's record): the result is the encoder's frame of the data.
 *
 * *d_status is the first of these that applies, and with ANY non-zero status not one byte of d_new_frame is written:
 *   1. the frame's own status: the checks of sqz_hip_frame_gather / _gather_dict in their order (the index checksum and
 *      the dictionary's length and CRC-32, EILSEQ, among them), then EINVAL for a frame whose win_bits is not the
 *      argument.  *d_blocks_encoded = 0.
 *   2. the touched block's errno: the decoder's, or EILSEQ for a checksum that does not hold.  The call does not build
 *      on content it cannot verify.
 *   3. the first encoder errno among the m blocks in ascending order, or EINVAL for a size that no index entry holds.
 *   4. E2BIG: the new frame does not fit capacity; *d_frame_bytes is the size it takes.
 *   *d_frame_bytes is the frame's size for status 0 and for 4, and 0 for 1 to 3.  *d_blocks_encoded is m in every case
 *   but 1.  A capacity of sqz_frame_bound / _bound_ex / _bound_dict of C + A for the frame's version is always enough.
 * EINVAL at the call, nothing enqueued: win_bits outside 10..15 or block_bits outside 12..24; n_blocks !=
 *   ceil(content_bytes / 2^block_bits); a null or misaligned d_frame, d_new_frame or d_scratch; a null d_frame_bytes,
 *   d_status or d_blocks_encoded; data_bytes > 0 with a null d_data; C + A overflowing, or a content that the frame
 *   bound answers 0 for; n' (or the m + 1 segments of the new payload) not fitting 32 bits; [d_new_frame, + capacity)
 *   overlapping [d_frame, + avail), the data or the scratch; the data overlapping the scratch; a scratch smaller than
 *   the function says; a parse that is none; _dict: d_dict == NULL or dict_bytes outside 1 .. 2^win_bits - 1.  E2BIG
 *   when avail does not cover header and index (and record), ENODEV without a device (after the argument checks).
 * Scratch, with t and m as above, w = ceil(n_blocks / 32), D = dict_bytes (0 for versions 1 and 2), every term rounded
 * up to 256:
 *       sqz_hip_frame_append_scratch_bytes(n_blocks, C, A, b, D) =
 *           2 * (4 w + 4) + 256 + 8 + 2 * 24 + 4 * 12               [the open for a list of one block: bitmap and its
 *                                                                     prefix counts, control words, the list, two
 *                                                                     offsets and four masks and results for its slot]
 *           + (t + A + 16)                                          [the staging area; t only when the block is touched,
 *                                                                     16 alone for A == 0]
 *           + 2 * 8 (m + 1) + (8 m + 8) + 2 * (4 m + 4)             [the encoder's two offset lists, its sizes, errnos
 *                                                                     and the new checksums]
 *           + 8 (m + 2) + 2 * 8 (m + 1)                             [the segment table of m + 1 segments]
 *           + 256 + (D > 0 ? 256 + 2 * round_up_256(4 * (D + 64)) : 0)  [the verdict words, the dictionary's index]
 *           + m * sqz_bound(2^b)                                    [m slabs]
 *           + max(sqz_hip_decode_scratch_bytes(2, 2^b), sqz_hip_encode_scratch_bytes(m, m << b))
 *   (the encoder's scratch over the decoder's, which is done by then); 0 for a bad block_bits, D > 32767, or sizes that
 *   wrap.  The encoder's 8 bytes per input byte and the slabs' 2 make a 1 GiB append take about 11 GiB of scratch: a
 *   caller with less memory appends in pieces -- appends compose, two of them leave the frame of one append of the
 *   concatenation.                                                                                                    */
SQZ_API uint64_t sqz_hip_frame_append_scratch_bytes(uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                                                    uint32_t block_bits, uint64_t dict_bytes);
SQZ_API int sqz_hip_frame_append(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                 uint32_t win_bits, uint32_t block_bits, const void* d_data, uint64_t data_bytes,
                                 uint32_t parse, void* d_new_frame, uint64_t capacity, uint64_t* d_frame_bytes,
                                 uint32_t* d_blocks_encoded, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                                 void* stream);
SQZ_API int sqz_hip_frame_append_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                                      uint32_t win_bits, uint32_t block_bits, const void* d_data, uint64_t data_bytes,
                                      uint32_t parse, const void* d_dict, uint64_t dict_bytes, void* d_new_frame,
                                      uint64_t capacity, uint64_t* d_frame_bytes, uint32_t* d_blocks_encoded,
                                      int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* MANY frames in one call, for a caller whose unit is the frame itself: one file per sample, per tensor, per shard.  A
 * frame call costs about one block's dependent chain whether it holds one block or thousands; k frames in one call run
 * their blocks through ONE launch chain, and the number of launches does not depend on k.  Device pointers; d_frames,
 * d_scratch 16-byte aligned; asynchronous, no host synchronisation inside.  Versions 1 and 2 only.  There is no format
 * change: every frame a batch writes is byte for byte the frame sqz_hip_frame_encode_parse writes for the same content
 * and arguments, and what a batch decodes is what sqz_hip_frame_decode delivers.  A frame that is refused or fails costs
 * that frame alone: its neighbours are written or delivered as if it were not there.
 *
 * ENCODE.  content_bytes: a HOST array of k sizes, brought to the device by one asynchronous copy on `stream` in front
 * of the first kernel (the array must stay as it is until that copy has run); the contents lie back to back in d_in.
 * One win_bits, block_bits, flags (0 or SQZ_FRAME_STORED) and parse for the call.  Frame f is written at d_frames +
 * frame_at[f], frame_at[f] = the sum over g < f of sqz_frame_bound_ex(content_bytes[g], block_bits, flags) rounded up
 * to 16; sqz_hip_frames_bound returns frame_at[k] (and the k + 1 offsets when frame_at is not NULL), 0 for parameters
 * out of range or sizes that wrap.  d_frame_bytes[f] and d_status[f] (k entries each) are the single call's: the status
 * is 0 or the first failed block's errno, and then nothing of that frame is written.  d_err has one entry per block of
 * the whole batch, frame f's from sum(n_blocks[g], g < f) on.  Bytes between the end of a frame and frame_at[f + 1] are
 * not touched.  An empty content gives the 32-byte frame.
 * EINVAL at the call, nothing enqueued: flags with another bit, a parse that is none, win_bits outside 10..15 or
 *   block_bits outside 12..24; a null content_bytes, d_frames, d_frame_bytes, d_status or d_scratch, a null d_in or
 *   d_err where there is content; d_frames or d_scratch misaligned; capacity below sqz_hip_frames_bound (so no frame
 *   can fail to fit); total blocks + k above 2^31 - 1; a scratch smaller than the function says.  k == 0 returns 0 and
 *   enqueues nothing.  ENODEV without a device (after the argument checks).
 * Scratch, with T = total blocks, S = total content, b = block_bits, every term rounded up to 256:
 *       sqz_hip_frames_encode_scratch_bytes = 8 k + 2 * 8 (k + 1) + 4 (k + 1)     [sizes; in_at, frame_at; first blocks]
 *           + 2 * 8 (T + 1) + (4 T + 4) + 2 * 8 T                   [the encoder's two offset lists, the checksums,
 *                                                                     stream sizes and copy sizes]
 *           + 8 (T + k) + 8 (T + 1) + (STORED ? 4 T + 4 : 0)        [dense offsets per frame and absolute, stored mask]
 *           + T * sqz_bound(2^b) + sqz_hip_encode_scratch_bytes(T, S); 0 for parameters out of range.
 *
 * DECODE.  items: a HOST array of k entries, what sqz_frame_info said about a host copy of each header (n_blocks,
 * content_bytes), where the frame lies in d_frames (frame_at, a multiple of 16; avail bytes of it are there) and where
 * its content goes in d_out (out_at); `zero` must be 0.  Any mix of versions 1 and 2, each frame with its own win_bits
 * and block_bits.  The table is brought to the device like the sizes of an encode.  d_status has k entries, d_err one per
 * block of the batch as above.  Per frame the checks are sqz_hip_frame_decode's in its order; a refused frame has its
 * status in d_status[f] and in every one of its d_err entries, none of its payload is read and none of its output is
 * written.  A frame of version 3 or 4 is refused in this way (EINVAL).  For an accepted frame d_err is what
 * sqz_hip_frame_decode leaves, EILSEQ for a block whose checksum does not hold included; its other blocks are delivered.
 * EINVAL at the call, nothing enqueued: a frame_at that is no multiple of 16; zero != 0; frames or outputs that are
 *   not ascending and disjoint (frame_at[f] + avail[f] <= frame_at[f + 1], out_at[f] + content_bytes[f] <=
 *   out_at[f + 1], neither sum wrapping); total blocks + k above 2^31 - 1; a null items, d_frames, d_status or
 *   d_scratch, a null d_out or d_err where there are blocks; d_frames or d_scratch misaligned; a scratch smaller than
 *   the function says.  E2BIG when an avail is below 32 + 8 n_blocks.  k == 0 returns 0 and enqueues nothing.  ENODEV
 *   without a device (after the argument checks).
 * Scratch, with T = total blocks, E = T + k entries (every frame has one more than blocks: a switched-off entry that
 * reaches over the next frame's header and index), X = out_at[k - 1] + content_bytes[k - 1] - out_at[0] (the decoder
 * keeps one word per byte of that span: gaps between outputs cost scratch), every term rounded up to 256:
 *       sqz_hip_frames_decode_scratch_bytes = 40 k + 4 (k + 1) + 2 * 8 (E + 1) + 4 * (4 E + 4)
 *           + sqz_hip_decode_scratch_bytes(E, X); 0 for a table the call would refuse.                              */
struct sqz_frames_item {
    uint64_t frame_at, avail, content_bytes, out_at;
    uint32_t n_blocks, zero;
};
SQZ_API uint64_t sqz_hip_frames_bound(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits, uint32_t flags,
                                      uint64_t* frame_at /* k + 1 entries, may be NULL */);
SQZ_API uint64_t sqz_hip_frames_encode_scratch_bytes(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits,
                                                     uint32_t flags);
SQZ_API int sqz_hip_frames_encode(const void* d_in, const uint64_t* content_bytes, uint32_t k, uint32_t win_bits,
                                  uint32_t block_bits, uint32_t flags, uint32_t parse, void* d_frames, uint64_t capacity,
                                  uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err, void* d_scratch,
                                  uint64_t scratch_bytes, void* stream);
SQZ_API uint64_t sqz_hip_frames_decode_scratch_bytes(const struct sqz_frames_item* items, uint32_t k);
SQZ_API int sqz_hip_frames_decode(const void* d_frames, const struct sqz_frames_item* items, uint32_t k, void* d_out,
                                  int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                                  void* stream);

/* Batches with byte-shuffled (version 4) frames: the calls above with one element size per frame, for a set of tensors
 * -- many frames of numeric data whose element size differs from one to the next.  The five calls above keep their
 * behaviour, their refusal of version 4 included; these are opt-in.  Everything said above holds unless said otherwise.
 *
 * ENCODE.  elem_bytes: a HOST array of k words, each 0, 2, 4 or 8, brought to the device by a second asynchronous copy
 * under content_bytes' lifetime rule.  Frame f is byte for byte what the single call writes for that content:
 * sqz_hip_frame_encode_parse for elem_bytes[f] == 0 (version 1 or 2), sqz_hip_frame_encode_shuf with elem_bytes[f]
 * otherwise (version 4, flags bit 2 set in the header; `flags` itself is 0 or SQZ_FRAME_STORED as above).  Status and
 * d_err are the single call's too: a frame whose shuffled bytes the block encoder refuses (E2BIG from the emit
 * kernel's tree guard) is refused alone.  frame_at[f] = the sum over g < f of sqz_frame_bound_shuf(content_bytes[g],
 * block_bits, flags | SQZ_FRAME_SHUFFLE) where elem_bytes[g] != 0 and of sqz_frame_bound_ex(..) where it is 0, each
 * rounded up to 16; sqz_hip_frames_bound_shuf returns frame_at[k], and 0 in addition for a null elem_bytes or a value
 * that is none of the four.  The contents are shuffled (or, for the frames with 0, copied) into the scratch by ONE
 * launch, and the block encoder reads them there; checksums and stored blocks are taken from d_in.  The number of
 * launches does not depend on k.  When every elem_bytes[f] is 0 the call enqueues exactly what sqz_hip_frames_encode
 * enqueues and needs exactly its scratch.
 * EINVAL at the call, nothing enqueued: everything sqz_hip_frames_encode refuses; a null elem_bytes; a value that is
 *   none of 0, 2, 4, 8.  k == 0 returns 0.  ENODEV after the argument checks.
 * Scratch, when one elem_bytes[f] at least is not 0 (S = total content, T = total blocks, every term rounded up to 256):
 *       sqz_hip_frames_encode_scratch_bytes_shuf = sqz_hip_frames_encode_scratch_bytes(content_bytes, k, b, flags)
 *           + 4 k + (4 T + 4) + (S + 16)      [element sizes per frame and per block; the content as the encoder reads it]
 *   and sqz_hip_frames_encode_scratch_bytes(..) itself when all are 0; 0 for parameters out of range.
 *
 * DECODE.  The same sqz_frames_item; for these two calls its last word carries the frame's elem_bytes: 0 for a frame
 * of version 1 or 2, else what sqz_frame_elem said about a host copy of header, index and record (2, 4 or 8).  Any mix
 * of versions 1, 2 and 4.  Per frame the checks are sqz_hip_frame_decode_shuf's for a version-4 header and
 * sqz_hip_frame_decode's for the others, in their order; the record must equal the item's elem_bytes.  A version-1 or
 * version-2 frame for which the item names an element size, a version-4 frame for which it names none, and a version-3
 * frame are refused (EINVAL), each alone, as above.  The decoder's output lies in the scratch; ONE launch writes the
 * blocks that are not stored into d_out, shuffled back by their frame's element size or copied; stored blocks are copied
 * from the frames and the checksums are taken over d_out.  When every item's element size is 0 the call enqueues what
 * sqz_hip_frames_decode enqueues and needs its scratch.
 * EINVAL at the call, nothing enqueued: everything sqz_hip_frames_decode refuses, with "a last word that is none of 0,
 *   2, 4, 8" in the place of "zero != 0".  E2BIG when an avail is below 32 + 8 n_blocks, or below 32 + 8 n_blocks + 8
 *   where an element size is named (the record).
 * Scratch, when one element size at least is not 0 (E, X as above, every term rounded up to 256):
 *       sqz_hip_frames_decode_scratch_bytes_shuf = sqz_hip_frames_decode_scratch_bytes(the items with 0 as last word, k)
 *           + (4 E + 4) + (X + 16)            [element size per entry; the span of the outputs as the decoder leaves it]
 *   and sqz_hip_frames_decode_scratch_bytes(..) itself when all are 0; 0 for a table the call would refuse.
 *
 * sqz_hip_shuffle_ranges is the pass on its own, sqz_hip_shuffle_blocks with one element size per range: d_elem[b]
 * (DEVICE array of n words) = 2, 4 or 8 transforms range b as sqz_hip_shuffle_blocks would with that size, 0 copies it
 * as it is; any other value, like d_skip[b] != 0 (d_skip may be NULL), leaves the range alone.                       */
SQZ_API uint64_t sqz_hip_frames_bound_shuf(const uint64_t* content_bytes, const uint32_t* elem_bytes, uint32_t k,
                                           uint32_t block_bits, uint32_t flags,
                                           uint64_t* frame_at /* k + 1 entries, may be NULL */);
SQZ_API uint64_t sqz_hip_frames_encode_scratch_bytes_shuf(const uint64_t* content_bytes, const uint32_t* elem_bytes,
                                                          uint32_t k, uint32_t block_bits, uint32_t flags);
SQZ_API int sqz_hip_frames_encode_shuf(const void* d_in, const uint64_t* content_bytes, const uint32_t* elem_bytes,
                                       uint32_t k, uint32_t win_bits, uint32_t block_bits, uint32_t flags, uint32_t parse,
                                       void* d_frames, uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status,
                                       int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream);
SQZ_API uint64_t sqz_hip_frames_decode_scratch_bytes_shuf(const struct sqz_frames_item* items, uint32_t k);
SQZ_API int sqz_hip_frames_decode_shuf(const void* d_frames, const struct sqz_frames_item* items, uint32_t k, void* d_out,
                                       int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                                       void* stream);
SQZ_API int sqz_hip_shuffle_ranges(const void* d_in, const uint64_t* d_off, const uint32_t* d_elem, uint32_t n,
                                   int inverse, void* d_out, const uint32_t* d_skip, void* stream);
/* What sqz_hip_shuffle_ranges replaces, for measuring against it (tools/microbench/frames_shuffle_batch_bench.py): ONE
 * element size and a mask.  elem_bytes 2, 4 or 8: sqz_hip_shuffle_blocks over the ranges with d_mask[b] == 0, the others
 * left alone; elem_bytes 0: the ranges with d_mask[b] != 0 copied as they are, the others left alone (the copy of stored
 * blocks, whose mask says which to take).  A mixed batch is up to three calls of the first kind and one of the second. */
SQZ_API int sqz_hip_shuffle_blocks_masked(const void* d_in, const uint64_t* d_off, uint32_t n, uint32_t elem_bytes,
                                          int inverse, void* d_out, const uint32_t* d_mask, void* stream);

/* Live timing of the last kernels enqueued through this library on the
 * calling thread's context, measured with HIP events ON THE LAUNCH STREAM.
 * Enabled with sqz_hip_set_timing(1); values in milliseconds.               */
enum {
    SQZ_HIP_K_LZ77_SCAN = 0,      /* lz77_scan_kernel (brute-force finder)            */
    SQZ_HIP_K_HUFFMAN_EMIT = 1,   /* huffman_emit_kernel                              */
    SQZ_HIP_K_ENTROPY_DECODE = 2, /* entropy_decode_kernel                            */
    SQZ_HIP_K_INDEX_SORT = 3,     /* index_sort_kernel   } indexed finder; a _dict encode call also sorts its dictionary
                                   * under this slot: two launches per call, their times summed (no slot is free for
                                   * dict_match_kernel, which is not timed here)                                      */
    SQZ_HIP_K_INDEX_MATCH = 4,    /* index_match_kernel  }                            */
    SQZ_HIP_K_INDEX_PARSE = 5,    /* index_parse_kernel  }                            */
    SQZ_HIP_K_LZ_EXPAND = 6,      /* lz_expand_kernel                                 */
    SQZ_HIP_K_RC_ENCODE = 7,      /* rc_encode_kernel  } R-era range coder            */
    SQZ_HIP_K_RC_DECODE = 8,      /* rc_decode_kernel  } (include/sqz/sqz_rc.h)       */
    SQZ_HIP_K_CRC32 = 9,          /* crc32_blocks_kernel } SQZF frames                */
    SQZ_HIP_K_FRAME_INDEX = 10,   /* frame_index_kernel / frame_open_kernel } (and an update's or append's planning) */
    SQZ_HIP_K_RANGE_COPY = 11,    /* range_copy_kernel: stored blocks (SQZF version 2); frame_splice_kernel */
    SQZ_HIP_KERNELS = 12
};
typedef struct sqz_hip_timing {
    float    ms[SQZ_HIP_KERNELS];        /* summed launch durations per kernel        */
    uint32_t launches[SQZ_HIP_KERNELS];
} sqz_hip_timing;
SQZ_API void sqz_hip_set_timing(int enabled);
SQZ_API int  sqz_hip_get_timing(sqz_hip_timing* out, int reset);

/* device / build information; returns 0 when a gfx950 device is usable */
SQZ_API int sqz_hip_device_info(char* name, size_t name_cap, int* compute_units,
                                uint64_t* lds_bytes_per_cu);
SQZ_API const char* sqz_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SQZ_AMD_SQZ_H */
