// sqz_amd/csrc/abi.hip -- the C ABI of libsqz_amd.so (include/sqz/sqz.h).
//
// Host side of the drop-in boundary: argument checks
// with the reference's errno conventions, H2D / D2H staging for the host
// flavour, kernel launches for the device flavour.  There is no CPU code path
// for the codec itself: without a gfx950 device every call reports ENODEV.
#include "../../include/sqz/sqz.h"
#include "../../include/sqz/sqz_rc.h"
#include "sqz_kernels.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

namespace {

constexpr uint64_t kMaxStream = 1ull << 31;     // per-stream limit (32-bit freq/tokens)
// a gather whose max_length is at most this copies with gather_copy_kernel (16 lanes per range), a longer one with
// range_copy_kernel (a workgroup per range): DESIGN.md section 10, "Gather", has the measurement
constexpr uint64_t sqzk_gather_copy_max = 4096;
constexpr uint32_t sqzk_max_window = 1u << sqz_max_win_bits;   // a decode call has no window: the largest one bounds its dictionary

// ---------------------------------------------------------------- device ctx
struct DevBuf {
    void*  p = nullptr;
    size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) { return 0; }
        if (p != nullptr) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = n + n / 4 + 4096;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            if (hipMalloc(&p, n) != hipSuccess) { p = nullptr; return ENOMEM; }
            want = n;
        }
        cap = want;
        return 0;
    }
};

struct Ctx {
    std::mutex mu;                  // guards the probe only: no call holds it while the device works
    int  state = 0;                 // 0 = unprobed, 1 = ok, -1 = no device
    char name[256] = {0};
    int  cus = 0;
    uint64_t lds = 0;
};

Ctx& ctx() { static Ctx c; return c; }

// Staging of the host-buffer flavour: one LANE per call in flight -- grow-only device buffers and a
// HIP stream of its own (SURVEY.md section 8b "Threading": one stream per call or caller-provided).
// A call leases a lane for its H2D -> kernels -> D2H and hands it back; concurrent callers get
// different lanes, so two threads neither serialise on a lock nor share the NULL stream.
struct Lane {
    hipStream_t own = nullptr;      // created with the lane (non-blocking: independent of the NULL stream)
    int device = -1;                // hipGetDevice() when the lane was made: its buffers and stream live there
    DevBuf in, out, in_off, out_off, tokens, tok_count, out_bytes, err, end_bit, work_a, work_m,
           dense, dense_off, crc, misc, dict, dict_idx, mask, shuf;
    std::vector<uint8_t> host_dense;   // landing area of the host flavour's one device-to-host copy
};

struct LanePool {
    std::mutex mu;
    std::vector<Lane*> idle;
    std::atomic<int> made{0};
};
LanePool& lanes() { static LanePool p; return p; }

struct LaneLease {
    Lane* lane = nullptr;
    LaneLease() {
        LanePool& p = lanes();
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) { dev = -1; }
        {
            // only a lane of the CURRENT device: another device's buffers and stream are of no use here
            std::lock_guard<std::mutex> g(p.mu);
            for (size_t k = p.idle.size(); k-- > 0;) {
                if (p.idle[k]->device == dev) { lane = p.idle[k]; p.idle.erase(p.idle.begin() + (long)k); break; }
            }
        }
        if (lane == nullptr) {
            lane = new Lane();
            lane->device = dev;
            if (hipStreamCreateWithFlags(&lane->own, hipStreamNonBlocking) != hipSuccess) { lane->own = nullptr; }
            p.made.fetch_add(1);
        }
    }
    ~LaneLease() {
        LanePool& p = lanes();
        std::lock_guard<std::mutex> g(p.mu);
        p.idle.push_back(lane);
    }
    // the caller's stream (struct sqz.stream) when given, else the lane's own
    hipStream_t stream(void* callers) const { return callers != nullptr ? (hipStream_t)callers : lane->own; }
};

int probe_locked(Ctx& c) {
    if (c.state != 0) { return c.state > 0 ? 0 : ENODEV; }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { c.state = -1; return ENODEV; }
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { c.state = -1; return ENODEV; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "libsqz_amd: device '%s' is not gfx950; kernels are built for "
                        "MI355X only\n", prop.gcnArchName);
        c.state = -1;
        return ENODEV;
    }
    snprintf(c.name, sizeof(c.name), "%s (%s)", prop.name, prop.gcnArchName);
    c.cus = prop.multiProcessorCount;
    c.lds = (uint64_t)prop.maxSharedMemoryPerMultiProcessor;
    c.state = 1;
    return 0;
}

int device_ready(void) {
    Ctx& c = ctx();
    std::lock_guard<std::mutex> g(c.mu);
    return probe_locked(c);
}

int hip_errno(hipError_t e) {
    if (e == hipSuccess) { return 0; }
    if (e == hipErrorOutOfMemory) { return ENOMEM; }
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) { return ENODEV; }
    fprintf(stderr, "libsqz_amd: HIP error %d (%s)\n", (int)e, hipGetErrorString(e));
    return EIO;
}

#define HIP_TRY(expr) do { const int _e = hip_errno(expr); if (_e != 0) { return _e; } } while (0)

// ---------------------------------------------------------------- timing
struct TimedSpan { hipEvent_t a, b; int kind; };
struct Timing {
    std::mutex mu;
    bool enabled = false;
    std::vector<TimedSpan> spans;
    sqz_hip_timing acc = {};
    // fold finished spans into acc and release their events (caller holds mu)
    void drain_locked() {
        for (TimedSpan& s : spans) {
            float ms = 0.0f;
            if (hipEventSynchronize(s.b) == hipSuccess && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
                if (s.kind >= 0 && s.kind < SQZ_HIP_KERNELS) { acc.ms[s.kind] += ms; acc.launches[s.kind]++; }
            }
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
        spans.clear();
    }
};
Timing& timing() { static Timing t; return t; }
constexpr size_t kMaxPendingSpans = 4096;       // a caller that never reads the timing must not grow it forever

struct SpanGuard {
    hipStream_t s; int kind; hipEvent_t a = nullptr, b = nullptr; bool on = false;
    SpanGuard(hipStream_t stream, int k) : s(stream), kind(k) {
        Timing& t = timing();
        std::lock_guard<std::mutex> g(t.mu);
        on = t.enabled;
        if (on) {
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            (void)hipEventRecord(a, s);
        }
    }
    ~SpanGuard() {
        if (!on) { return; }
        (void)hipEventRecord(b, s);
        Timing& t = timing();
        std::lock_guard<std::mutex> g(t.mu);
        t.spans.push_back({a, b, kind});
        if (t.spans.size() >= kMaxPendingSpans) { t.drain_locked(); }
    }
};

// ---------------------------------------------------------------- host bit I/O
// bitstream.h:28-63 / :65-103, both modes, used only for the stream headers.
bool writer_is_memory(const bitstream* bs) { return bs->data != NULL && bs->capacity > 0; }     // bitstream.h:34
bool writer_is_callback(const bitstream* bs) { return bs->data == NULL && bs->capacity == 0 && bs->output != NULL; }
bool reader_is_callback(const bitstream* bs) { return bs->data == NULL && bs->bytes == 0 && bs->input != NULL; }

void host_put_bit(bitstream* bs, int bit) {
    if (bs->error != 0) { return; }
    bs->b64 = (bs->b64 << 1) | (uint64_t)(bit & 1);
    if (++bs->bits == 64) {
        if (writer_is_memory(bs)) {
            for (int k = 0; k < 8 && bs->error == 0; k++) {
                if (bs->bytes == bs->capacity) { bs->error = E2BIG; }
                else { bs->data[bs->bytes++] = (uint8_t)(bs->b64 >> (56 - 8 * k)); }
            }
        } else if (writer_is_callback(bs)) {                    // bitstream.h:44-48
            bs->error = bs->output(bs);
            if (bs->error == 0) { bs->bytes += 8; }
        } else {
            bs->error = EINVAL;
        }
        bs->bits = 0;
        bs->b64 = 0;
    }
}

void host_put_bits(bitstream* bs, uint64_t v, int n) {
    for (int b = 0; b < n && bs->error == 0; b++) { host_put_bit(bs, (int)((v >> b) & 1)); }
}

uint64_t reader_limit(const bitstream* bs) { return bs->bytes != 0 ? bs->bytes : bs->capacity; }

int host_get_bit(bitstream* bs) {
    if (bs->error != 0) { return 0; }
    if (bs->bits == 0) {
        bs->b64 = 0;
        if (bs->data != NULL) {
            const uint64_t limit = reader_limit(bs);
            for (int k = 0; k < 8 && bs->error == 0; k++) {
                if (bs->read == limit) { bs->error = E2BIG; }
                else { bs->b64 |= (uint64_t)bs->data[bs->read++] << (56 - 8 * k); }
            }
        } else if (reader_is_callback(bs)) {                    // bitstream.h:81-85
            bs->error = bs->input(bs);
            if (bs->error == 0) { bs->read += 8; }
        } else {
            bs->error = EINVAL;
        }
        bs->bits = 64;
    }
    const int bit = (int)(bs->b64 >> 63);
    bs->b64 <<= 1;
    bs->bits--;
    return bit;
}

uint64_t host_get_bits(bitstream* bs, int n) {
    uint64_t v = 0;
    for (int b = 0; b < n && bs->error == 0; b++) { v |= (uint64_t)host_get_bit(bs) << b; }
    return v;
}

uint64_t load_be64(const uint8_t* p) {
    uint64_t w = 0;
    for (int k = 0; k < 8; k++) { w = (w << 8) | p[k]; }
    return w;
}

void store_be64(uint8_t* p, uint64_t w) {
    for (int k = 0; k < 8; k++) { p[k] = (uint8_t)(w >> (56 - 8 * k)); }
}

bool window_ok(uint32_t w) { return w >= 2 && w <= 32768; }

// wavefronts that share one stream's LDS window in the scan kernel (tuning knob:
// SQZ_SCAN_WAVES=1|2|4|8, default 4 = four waves on every SIMD at 4 streams per CU)
int scan_waves() {
    static const int w = [] {
        const char* e = getenv("SQZ_SCAN_WAVES");
        const int v = e != NULL ? atoi(e) : 4;
        return (v == 1 || v == 2 || v == 4 || v == 8) ? v : 4;
    }();
    return w;
}

int check_offsets(const uint64_t* off, uint32_t n, bool need8) {
    for (uint32_t b = 0; b < n; b++) {
        if (off[b + 1] < off[b] || off[b + 1] - off[b] > kMaxStream) { return EINVAL; }
        if (need8 && (off[b] & 7u) != 0) { return EINVAL; }
    }
    return 0;
}

uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// match finder of encode stage 1: 1 = indexed (default), 0 = brute-force scan
// (SQZ_FINDER=scan|index).  Both produce the reference's tokens.
std::atomic<int> g_finder{-1};      // -1 = not chosen yet
int finder_default() {
    int f = g_finder.load(std::memory_order_relaxed);
    if (f < 0) {
        const char* e = getenv("SQZ_FINDER");
        const int chosen = (e != NULL && strcmp(e, "scan") == 0) ? 0 : 1;
        // a concurrent sqz_hip_set_finder wins over the environment's default
        f = g_finder.compare_exchange_strong(f, chosen) ? chosen : g_finder.load();
    }
    return f;
}

// Wavefronts per stream in the entropy decoder.  A batch of more than 4 streams per CU runs one wave per
// stream (16 streams per CU fit: the batch fills the chip by itself); smaller batches leave SIMDs idle and the
// decoder spends them on the read-ahead: 4 waves per stream up to 4 streams per CU, 8 up to 2 (measured,
// MI355X, entropy_decode_kernel: 512 blocks 62.4 -> 51.4 -> 49.4 ms with 1 / 4 / 8 waves, 1024 blocks
// 63.6 -> 54.0 ms with 4; 2 waves per stream gain 2-4 % at best and lose at 2048 blocks: not taken).
// SQZ_DECODE_WAVES=1|2|4|8 overrides.
int decode_waves_for(uint32_t n_blocks) {
    static const int forced = [] { const char* e = getenv("SQZ_DECODE_WAVES"); return e != NULL ? atoi(e) : 0; }();
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) { return forced; }
    int cus = ctx().cus;
    if (cus <= 0) { cus = 256; }
    if ((uint64_t)n_blocks <= (uint64_t)cus * 2) { return 8; }
    return (uint64_t)n_blocks <= (uint64_t)cus * 4 ? 4 : 1;
}

uint32_t match_groups_for(uint64_t avg_block_bytes) {
    static const int div = [] { const char* e = getenv("SQZ_MATCH_DIV"); const int v = e != NULL ? atoi(e) : 1024; return v >= 256 ? v : 1024; }();
    uint64_t g = (avg_block_bytes + div - 1) / div;
    if (g < 1) { g = 1; }
    if (g > 65535) { g = 65535; }
    return (uint32_t)g;
}

bool parse_ok(uint32_t parse) { return parse == SQZ_PARSE_GREEDY || parse == SQZ_PARSE_LAZY; }
// the lazy parse reads the match table, which only the indexed finder writes: it runs that finder whatever is set
int finder_for(uint32_t parse) { return parse == SQZ_PARSE_LAZY ? 1 : finder_default(); }

// A call's shared dictionary on the device: its bytes and, for an encode, its positions sorted by 3-byte prefix.
struct DictDev { const uint8_t* bytes = nullptr; uint32_t len = 0; const uint32_t* sorted = nullptr; };
bool dict_ok(const void* dict, uint64_t dict_bytes, uint32_t window) {
    return dict != NULL && dict_bytes >= 1 && window >= 2 && dict_bytes <= (uint64_t)window - 1;
}
// what the dictionary's index takes of an encode's scratch: the sort's one-block offsets and its two buffers
uint64_t dict_slot_bytes(uint64_t dict_bytes) { return align_up((dict_bytes + 64) * 4, 256); }
uint64_t dict_index_bytes(uint64_t dict_bytes) { return 256 + 2 * dict_slot_bytes(dict_bytes); }
// index_sort_kernel on the dictionary as a one-block batch, once per call; area: dict_index_bytes, 16-byte aligned
DictDev run_dict_index(const uint8_t* d_dict, uint32_t dict_bytes, uint8_t* area, hipStream_t st) {
    uint64_t* const off = (uint64_t*)area;                   // {0, D}, written on the device: no host copy to wait for
    uint32_t* const a = (uint32_t*)(area + 256);
    uint32_t* const b = (uint32_t*)(area + 256 + dict_slot_bytes(dict_bytes));
    sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, off, off + 4, st);
    SpanGuard g(st, SQZ_HIP_K_INDEX_SORT);
    sqzk::launch_index_sort(d_dict, off, 1, a, b, (uint64_t)dict_bytes + 64, st);
    DictDev dd;
    dd.bytes = d_dict; dd.len = dict_bytes; dd.sorted = a;
    return dd;
}
// the host flavour: the caller's dictionary into the lane's buffers, indexed when the call encodes
int upload_dict(Lane& c, hipStream_t st, const uint8_t* dict, uint32_t dict_bytes, bool index, DictDev* dd) {
    int e;
    if ((e = c.dict.reserve((size_t)dict_bytes + 16)) || (index && (e = c.dict_idx.reserve(dict_index_bytes(dict_bytes))))) {
        return e;
    }
    HIP_TRY(hipMemcpyAsync(c.dict.p, dict, dict_bytes, hipMemcpyHostToDevice, st));
    if (index) {
        *dd = run_dict_index((const uint8_t*)c.dict.p, dict_bytes, (uint8_t*)c.dict_idx.p, st);
    } else {
        dd->bytes = (const uint8_t*)c.dict.p; dd->len = dict_bytes; dd->sorted = nullptr;
    }
    return 0;
}

// stage 1 on device buffers -> token words; work = 2 arrays of one uint32 slot per input byte
// (parse = SQZ_PARSE_LAZY: finder 1 and both work arrays, the callers see to that)
void run_stage1(int finder, const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n,
                uint32_t window, uint32_t* tokens, uint32_t* counts,
                uint32_t* work_a, uint32_t* work_m, uint64_t avg_block, uint64_t slots,
                hipStream_t st, uint32_t parse = SQZ_PARSE_GREEDY, const DictDev* dd = nullptr) {
    if (finder == 0 || work_a == nullptr || work_m == nullptr) {
        SpanGuard g(st, SQZ_HIP_K_LZ77_SCAN);
        sqzk::launch_lz77_scan(d_in, d_in_off, n, window, tokens, counts, scan_waves(), slots, st);
    } else {
        { SpanGuard g(st, SQZ_HIP_K_INDEX_SORT);
          // two arrays serve the three steps: the sort leaves the positions in work_a (work_m is its second
          // buffer), the match table goes to work_m (the sort is done with it), and the token words may take
          // work_a's place (tokens == work_a in the encode path: the sorted positions are dead by then)
          sqzk::launch_index_sort(d_in, d_in_off, n, work_a, work_m /* ping-pong */, slots, st); }
        { SpanGuard g(st, SQZ_HIP_K_INDEX_MATCH);
          sqzk::launch_index_match(d_in, d_in_off, n, window, work_a, work_m,
                                   match_groups_for(avg_block), slots, st); }
        if (dd != nullptr) {                                    // (no slot of sqz_hip_timing is free: not timed here)
            sqzk::launch_dict_match(d_in, d_in_off, n, window, dd->bytes, dd->len, dd->sorted, work_m, slots, st);
        }
        { SpanGuard g(st, SQZ_HIP_K_INDEX_PARSE);
          if (parse == SQZ_PARSE_LAZY) {
              sqzk::launch_index_parse_lazy(d_in, d_in_off, n, work_m, tokens, counts, slots, st);
          } else {
              sqzk::launch_index_parse(d_in, d_in_off, n, work_m, tokens, counts, slots, st);
          } }
    }
}

// the whole encode on device buffers: stage 1 (either finder) -> token words -> emit
void run_encode(int finder, const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n,
                uint32_t window, uint32_t* tokens, uint32_t* counts, uint32_t* work_a,
                uint32_t* work_m, uint64_t avg_block, uint8_t* d_out, const uint64_t* d_out_off,
                uint64_t* d_out_bytes, int32_t* d_err, uint64_t prefix_acc, int prefix_fill,
                uint64_t slots, sqz_block_stats* d_stats, hipStream_t st, uint32_t parse = SQZ_PARSE_GREEDY,
                const DictDev* dd = nullptr) {
    run_stage1(finder, d_in, d_in_off, n, window, tokens, counts, work_a, work_m, avg_block, slots, st, parse, dd);
    SpanGuard g(st, SQZ_HIP_K_HUFFMAN_EMIT);
    sqzk::launch_huffman_emit(tokens, d_in_off, counts, d_out, d_out_off, d_out_bytes, d_err, n,
                              prefix_acc, prefix_fill, d_stats, st);
}

// host-buffer encode of n blocks; prefix = pending header bits of block 0
// (single-stream API only).  `c` is the caller's leased lane, `st` the stream of this call.
int encode_host(Lane& c, hipStream_t st, const uint8_t* in, const uint64_t* in_off, uint32_t n,
                       uint32_t window, uint8_t* out, const uint64_t* out_off,
                       uint64_t* out_bytes, int32_t* err,
                       uint64_t prefix_acc, int prefix_fill, uint64_t* tokens_total,
                       uint32_t parse = SQZ_PARSE_GREEDY, const uint8_t* dict = nullptr, uint32_t dict_bytes = 0) {
    const uint64_t in_base = in_off[0], out_base = out_off[0];
    const uint64_t total_in = in_off[n] - in_base, total_out = out_off[n] - out_base;
    std::vector<uint64_t> io(n + 1), oo(n + 1);
    for (uint32_t b = 0; b <= n; b++) { io[b] = in_off[b] - in_base; oo[b] = out_off[b] - out_base; }

    int e;
    if ((e = c.in.reserve(total_in + 16)) || (e = c.out.reserve(total_out + 16)) ||
        (e = c.in_off.reserve((n + 1) * 8)) || (e = c.out_off.reserve((n + 1) * 8)) ||
        (e = c.tok_count.reserve((size_t)n * 4)) ||
        (e = c.work_a.reserve((total_in + 64) * 4)) || (e = c.work_m.reserve((total_in + 64) * 4)) ||
        (e = c.out_bytes.reserve((size_t)n * 8)) || (e = c.err.reserve((size_t)n * 4))) {
        return e;
    }
    if (total_in > 0) { HIP_TRY(hipMemcpyAsync(c.in.p, in + in_base, total_in, hipMemcpyHostToDevice, st)); }
    HIP_TRY(hipMemcpyAsync(c.in_off.p, io.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.out_off.p, oo.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    uint64_t widest = 0;
    for (uint32_t b = 0; b < n; b++) { widest = io[b + 1] - io[b] > widest ? io[b + 1] - io[b] : widest; }
    DictDev dd;
    if (dict != nullptr && (e = upload_dict(c, st, dict, dict_bytes, true, &dd)) != 0) { return e; }
    run_encode(dict != nullptr ? 1 : finder_for(parse), (const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, n, window,
               (uint32_t*)c.work_a.p /* token words take the sorted positions' place */, (uint32_t*)c.tok_count.p,
               (uint32_t*)c.work_a.p, (uint32_t*)c.work_m.p, widest, (uint8_t*)c.out.p, (const uint64_t*)c.out_off.p,
               (uint64_t*)c.out_bytes.p, (int32_t*)c.err.p, prefix_acc, prefix_fill, total_in + 64, nullptr, st, parse,
               dict != nullptr ? &dd : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_bytes, c.out_bytes.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(err, c.err.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the streams leave as ONE transfer: packed back to back on the device first (the slabs are
    // sized for the worst case, 2.3 x what a Zipf block produces), then spread over the caller's
    // slabs on the host.  Only out[out_off[b] .. + out_bytes[b]) is written.
    std::vector<uint64_t> dense_off(n + 1);
    dense_off[0] = 0;
    for (uint32_t b = 0; b < n; b++) { dense_off[b + 1] = dense_off[b] + ((out_bytes[b] + 7) & ~7ull); }
    const uint64_t dense_total = dense_off[n];
    if (dense_total > 0) {
        if (n == 1) {
            HIP_TRY(hipMemcpyAsync(out + out_off[0], c.out.p, out_bytes[0], hipMemcpyDeviceToHost, st));
        } else {
            if ((e = c.dense.reserve(dense_total + 16)) || (e = c.dense_off.reserve((n + 1) * 8))) { return e; }
            HIP_TRY(hipMemcpyAsync(c.dense_off.p, dense_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
            sqzk::launch_compact_blocks((const uint8_t*)c.out.p, (const uint64_t*)c.out_off.p,
                                        (const uint64_t*)c.out_bytes.p, n, (uint8_t*)c.dense.p,
                                        (const uint64_t*)c.dense_off.p, dense_total / n, st);
            HIP_TRY(hipGetLastError());
            if (c.host_dense.size() < dense_total) { c.host_dense.resize(dense_total); }
            HIP_TRY(hipMemcpyAsync(c.host_dense.data(), c.dense.p, dense_total, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint32_t b = 0; b < n; b++) {
                memcpy(out + out_off[b], c.host_dense.data() + dense_off[b], out_bytes[b]);
            }
        }
    }
    if (tokens_total != nullptr) {
        std::vector<uint32_t> tc(n);
        HIP_TRY(hipMemcpyAsync(tc.data(), c.tok_count.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uint64_t sum = 0;
        for (uint32_t b = 0; b < n; b++) { sum += tc[b]; }
        *tokens_total = sum;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int decode_host(Lane& c, hipStream_t st, const uint8_t* in, const uint64_t* in_off, uint32_t n,
                uint8_t* out, const uint64_t* out_off, int32_t* err,
                uint64_t start_bit, uint64_t* end_bit, const uint8_t* dict = nullptr, uint32_t dict_bytes = 0) {
    const uint64_t in_base = in_off[0], out_base = out_off[0];
    const uint64_t total_in = in_off[n] - in_base, total_out = out_off[n] - out_base;
    std::vector<uint64_t> io(n + 1), oo(n + 1);
    for (uint32_t b = 0; b <= n; b++) { io[b] = in_off[b] - in_base; oo[b] = out_off[b] - out_base; }
    int e;
    if ((e = c.in.reserve(total_in + 16)) || (e = c.out.reserve(total_out + 16)) ||
        (e = c.in_off.reserve((n + 1) * 8)) || (e = c.out_off.reserve((n + 1) * 8)) ||
        (e = c.err.reserve((size_t)n * 4)) || (e = c.end_bit.reserve((size_t)n * 8)) ||
        (e = c.tokens.reserve((total_out + 64) * 4)) || (e = c.tok_count.reserve((size_t)n * 4))) {
        return e;
    }
    if (total_in > 0) { HIP_TRY(hipMemcpyAsync(c.in.p, in + in_base, total_in, hipMemcpyHostToDevice, st)); }
    HIP_TRY(hipMemcpyAsync(c.in_off.p, io.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.out_off.p, oo.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    DictDev dd;
    if (dict != nullptr && (e = upload_dict(c, st, dict, dict_bytes, false, &dd)) != 0) { return e; }
    {
        SpanGuard g(st, SQZ_HIP_K_ENTROPY_DECODE);
        sqzk::launch_entropy_decode((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p,
                                    (const uint64_t*)c.out_off.p, (uint32_t*)c.tokens.p,
                                    (uint32_t*)c.tok_count.p, (int32_t*)c.err.p,
                                    (uint64_t*)c.end_bit.p, n, start_bit, decode_waves_for(n), st, nullptr, dd.len);
    }
    {
        SpanGuard g(st, SQZ_HIP_K_LZ_EXPAND);
        sqzk::launch_lz_expand((const uint32_t*)c.tokens.p, (const uint32_t*)c.tok_count.p,
                               (uint8_t*)c.out.p, (const uint64_t*)c.out_off.p, n, st, nullptr, dd.bytes, dd.len);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(err, c.err.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (total_out > 0) {
        HIP_TRY(hipMemcpyAsync(out + out_base, c.out.p, total_out, hipMemcpyDeviceToHost, st));
    }
    if (end_bit != nullptr) {
        HIP_TRY(hipMemcpyAsync(end_bit, c.end_bit.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}


// ---------------------------------------------------------------- SQZF frames (include/sqz/sqz.h)
static_assert(EINVAL == 22 && E2BIG == 7 && EILSEQ == 84, "frame.hip writes these errno values from the device");
static_assert(ENOBUFS == 105 && ENOSPC == 28, "frame.hip writes these errno values from the device");
static_assert(ERANGE == 34 && ENODATA == 61, "frame.hip writes these errno values from the device");

uint32_t get_le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t get_le64(const uint8_t* p) { return (uint64_t)get_le32(p) | ((uint64_t)get_le32(p + 4) << 32); }
void put_le32(uint8_t* p, uint32_t v) { for (int k = 0; k < 4; k++) { p[k] = (uint8_t)(v >> (8 * k)); } }
void put_le64(uint8_t* p, uint64_t v) { put_le32(p, (uint32_t)v); put_le32(p + 4, (uint32_t)(v >> 32)); }

// zlib's crc32 on the host (header and index only: 8 bytes per block); crc = 0 starts, a result continues
uint32_t host_crc32(uint32_t crc, const uint8_t* p, uint64_t n) {
    static const std::vector<uint32_t> table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) { c = (c >> 1) ^ ((0u - (c & 1u)) & 0xEDB88320u); }
            t[i] = c;
        }
        return t;
    }();
    crc = ~crc;
    for (uint64_t k = 0; k < n; k++) { crc = table[(crc ^ p[k]) & 0xFFu] ^ (crc >> 8); }
    return ~crc;
}

bool frame_params_ok(uint32_t win_bits, uint32_t block_bits) {
    return win_bits >= (uint32_t)sqz_min_win_bits && win_bits <= (uint32_t)sqz_max_win_bits &&
           block_bits >= (uint32_t)sqz_frame_min_block_bits && block_bits <= (uint32_t)sqz_frame_max_block_bits;
}
uint64_t frame_blocks(uint64_t content_bytes, uint32_t block_bits) {
    return (content_bytes >> block_bits) + ((content_bytes & ((1ull << block_bits) - 1)) != 0 ? 1 : 0);
}
// record: the 8 bytes { dict_bytes, dict_crc } behind the index of a version-3 frame, 0 otherwise
uint64_t frame_payload_off(uint64_t n_blocks, uint64_t record = 0) { return align_up(32 + 8 * n_blocks + record, 16); }
// content bytes of block b
uint64_t frame_block_len(uint64_t content_bytes, uint32_t block_bits, uint64_t b) {
    const uint64_t bb = 1ull << block_bits, at = b * bb;
    return at >= content_bytes ? 0 : (content_bytes - at < bb ? content_bytes - at : bb);
}
// block b's share of the payload in words: in version 2 bit 31 of the entry is the stored bit
uint32_t frame_entry_words(const uint8_t* frame, uint32_t version, uint64_t b) {
    const uint32_t e = get_le32(frame + 32 + 8 * b);
    return version >= 2 ? e & 0x7FFFFFFFu : e;
}
bool frame_entry_stored(const uint8_t* frame, uint32_t version, uint64_t b) {
    return version >= 2 && (get_le32(frame + 32 + 8 * b) >> 31) != 0;
}
bool frame_flags_ok(uint32_t flags) { return flags == 0 || flags == (uint32_t)SQZ_FRAME_STORED; }

// content bytes a host call works through per pass (whole blocks, one at least)
uint64_t frame_pass_blocks(uint64_t block_bytes) {
    uint64_t pass = 1ull << 30;
    const char* e = getenv("SQZ_FRAME_PASS_BYTES");         // read at every call: a test sets it low
    if (e != NULL && atoll(e) > 0) { pass = (uint64_t)atoll(e); }
    const uint64_t blocks = pass / block_bytes;
    return blocks < 1 ? 1 : (blocks > 0x7FFFFFFFull ? 0x7FFFFFFFull : blocks);
}

// where the pieces of a device call's scratch lie (every piece 256-byte aligned)
struct FrameScratch {
    uint64_t in_off, out_off, out_bytes, copy_bytes, dense_off, crc, misc, slabs, codec, codec_bytes, stored, shuf, total;
};
// store: an encode that may store blocks has a mask of its own.  A decode keeps its mask in `crc`: the open
// kernel writes it, the decode and copy kernels read it, and only then, on the same stream, do the checksums
// of the output land there -- so a decode of either version needs exactly the scratch it always did.
// shuf: version 4 keeps the shuffled content, round_up_256(content_bytes + 16) bytes, behind everything else -- an
// encode the whole content before the encoder reads it, a decode the selected blocks as the decoder leaves them
FrameScratch frame_scratch(uint64_t n, uint64_t content_bytes, uint64_t slab_bytes, bool encode, bool store = false,
                           bool shuf = false) {
    FrameScratch L = {};
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) { const uint64_t r = at; at += align_up(bytes, 256); return r; };
    L.in_off = take((n + 1) * 8);
    L.out_off = take((n + 1) * 8);                          // encode: the slabs' offsets
    L.crc = take(n * 4 + 4);
    L.misc = take(256);                                     // [0,16) the index's range, [16,20) its checksum, [32,48) spare;
                                                            // version 3: [64,80) the dictionary's range, [96,112) spare,
                                                            // [128,132) the dictionary's checksum
    if (encode) {
        L.out_bytes = take(n * 8);
        L.copy_bytes = take(n * 8);
        L.dense_off = take((n + 1) * 8);
        L.slabs = take(n * slab_bytes);
        L.codec_bytes = sqz_hip_encode_scratch_bytes((uint32_t)n, content_bytes);
    } else {
        L.codec_bytes = sqz_hip_decode_scratch_bytes((uint32_t)n, content_bytes);
    }
    L.codec = take(L.codec_bytes);
    L.stored = encode && store ? take(n * 4 + 4) : L.crc;
    L.shuf = shuf ? take(content_bytes + 16) : 0;
    L.total = at;
    return L;
}

// the device side of a frame encode: everything enqueued on st, nothing waits
int frame_encode_dev(const uint8_t* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                     uint8_t* d_frame, uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status,
                     int32_t* d_err, uint8_t* scratch, uint64_t scratch_bytes, hipStream_t st, uint32_t flags = 0,
                     uint32_t parse = SQZ_PARSE_GREEDY, const uint8_t* d_dict = nullptr, uint32_t dict_bytes = 0,
                     uint32_t elem = 0) {
    // elem: 2, 4 or 8 writes version 4 (never with a dictionary); 0 every other version as it always was
    const uint64_t bb = 1ull << block_bits, n64 = frame_blocks(content_bytes, block_bits);
    if (n64 > 0xFFFFFFFFull) { return EINVAL; }
    const uint32_t n = (uint32_t)n64;
    const uint64_t slab = sqz_bound(bb);
    const bool store = (flags & SQZ_FRAME_STORED) != 0;
    const FrameScratch L = frame_scratch(n, content_bytes, slab, true, store, elem != 0);
    // version 3: the dictionary's index lies in front of everything else, as in sqz_hip_encode_blocks_dict
    const uint64_t dict_area = d_dict != nullptr ? dict_index_bytes(dict_bytes) : 0;
    if (scratch_bytes < dict_area + L.total) { return EINVAL; }
    uint8_t* const dict_idx = scratch;
    scratch += dict_area;
    uint32_t* stored = (uint32_t*)(scratch + L.stored);
    uint64_t* in_off = (uint64_t*)(scratch + L.in_off);
    uint64_t* slab_off = (uint64_t*)(scratch + L.out_off);
    uint64_t* out_bytes = (uint64_t*)(scratch + L.out_bytes);
    uint64_t* copy_bytes = (uint64_t*)(scratch + L.copy_bytes);
    uint64_t* dense_off = (uint64_t*)(scratch + L.dense_off);
    uint32_t* crc = (uint32_t*)(scratch + L.crc);
    uint64_t* idx_off = (uint64_t*)(scratch + L.misc);
    uint32_t* idx_crc = (uint32_t*)(scratch + L.misc + 16);
    uint32_t* dict_crc = (uint32_t*)(scratch + L.misc + 128);
    sqzk::launch_frame_plan(n, bb, content_bytes, slab, in_off, slab_off, st);
    DictDev dd;
    if (d_dict != nullptr) {                                // sorted once per call; its checksum over the sort's own
        dd = run_dict_index(d_dict, dict_bytes, dict_idx, st);  // range {0, D}, for the record
        SpanGuard g(st, SQZ_HIP_K_CRC32);
        sqzk::launch_crc32_blocks(d_dict, (const uint64_t*)dict_idx, 1, dict_crc, dict_bytes, st);
    }
    if (n > 0) {
        { SpanGuard g(st, SQZ_HIP_K_CRC32);
          sqzk::launch_crc32_blocks(d_in, in_off, n, crc, bb, st); }
        const uint64_t head = align_up((uint64_t)n * 4, 256);
        const uint64_t slots = (L.codec_bytes - head) / 8;
        uint32_t* counts = (uint32_t*)(scratch + L.codec);
        uint32_t* tokens = (uint32_t*)(scratch + L.codec + head);
        const uint8_t* enc_in = d_in;                       // version 4: the encoder reads every block shuffled; checksum
        if (elem != 0) {                                    // (above) and stored blocks (below) keep to the caller's bytes
            sqzk::launch_shuffle_blocks(d_in, in_off, n, elem, false, scratch + L.shuf, nullptr, bb, st);
            enc_in = scratch + L.shuf;
        }
        run_encode(d_dict != nullptr ? 1 : finder_for(parse), enc_in, in_off, n, 1u << win_bits, tokens, counts, tokens,
                   tokens + slots, bb, scratch + L.slabs, slab_off, out_bytes, d_err, 0, 0, slots, nullptr, st, parse,
                   d_dict != nullptr ? &dd : nullptr);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      if (d_dict != nullptr) {
          sqzk::launch_frame_index_v3(out_bytes, d_err, crc, n, content_bytes, win_bits, block_bits, flags, dict_bytes,
                                      dict_crc, d_frame, capacity, copy_bytes, dense_off, stored, idx_off,
                                      d_frame_bytes, d_status, st);
      } else if (elem != 0) {
          sqzk::launch_frame_index_v4(out_bytes, d_err, crc, n, content_bytes, win_bits, block_bits, flags, elem, d_frame,
                                      capacity, copy_bytes, dense_off, stored, idx_off, d_frame_bytes, d_status, st);
      } else if (store) {
          sqzk::launch_frame_index_v2(out_bytes, d_err, crc, n, content_bytes, win_bits, block_bits, d_frame, capacity,
                                      copy_bytes, dense_off, stored, idx_off, d_frame_bytes, d_status, st);
      } else {
          sqzk::launch_frame_index(out_bytes, d_err, crc, n, content_bytes, win_bits, block_bits, d_frame, capacity,
                                   copy_bytes, dense_off, idx_off, d_frame_bytes, d_status, st);
      } }
    const uint32_t record = d_dict != nullptr || elem != 0 ? 8 : 0;
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(d_frame, idx_off, 1, idx_crc, 8 * (uint64_t)n + record, st); }
    sqzk::launch_frame_seal(d_frame, idx_crc, n, d_status, st, record);
    if (n > 0) {
        sqzk::launch_compact_blocks(scratch + L.slabs, slab_off, copy_bytes, n, d_frame, dense_off, bb / 2, st);
        if (store) {                                        // the stored blocks' content, where the index says
            SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
            sqzk::launch_range_copy(d_in, in_off, d_frame, dense_off, in_off, stored, n, true, bb, st);
        }
    }
    return hip_errno(hipGetLastError());
}

// What every frame decode enqueues for n selected blocks once their offsets (and the stored mask, `skip`, null: no
// block is stored) are on the device: entropy stage, expansion, the stored blocks' copy, the checksums of the output.
// dd: the shared dictionary of a version-3 frame (len 0: none).  Shared by the device-resident decode, whose offsets
// frame_open_kernel wrote, and the host decode of a version-3 frame, whose offsets the host worked out.
void run_frame_decode(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* out_off, uint32_t n,
                      uint64_t size_hint, uint32_t* tokens, uint32_t* counts, uint8_t* d_out, int32_t* d_err,
                      const uint32_t* skip, const uint32_t* stored, uint32_t* crc, const DictDev& dd, hipStream_t st,
                      uint32_t n_streams = 0, uint8_t* d_shuf = nullptr, uint32_t elem = 0,
                      const uint32_t* elems = nullptr) {
    // elems: a batch of frames -- one element size per entry in place of elem, 0 for an entry that is only copied
    // d_shuf, elem: version 4 -- the expansion writes the shuffled blocks there (same offsets), the inverse shuffle
    // brings every block that is not stored to d_out; stored blocks, checksums and verification then see d_out as ever
    // n_streams: how many of the n entries can be streams at all, where that is fewer (a gather's pseudo-blocks)
    { SpanGuard g(st, SQZ_HIP_K_ENTROPY_DECODE);
      sqzk::launch_entropy_decode(d_in, in_off, out_off, tokens, counts, d_err, nullptr, n, 0,
                                  decode_waves_for(n_streams != 0 ? n_streams : n), st, skip, dd.len); }
    { SpanGuard g(st, SQZ_HIP_K_LZ_EXPAND);
      sqzk::launch_lz_expand(tokens, counts, d_shuf != nullptr ? d_shuf : d_out, out_off, n, st, skip, dd.bytes, dd.len); }
    if (d_shuf != nullptr && elems != nullptr) {
        sqzk::launch_shuffle_ranges(d_shuf, out_off, elems, n, true, d_out, skip, size_hint, st);
    } else if (d_shuf != nullptr) {
        sqzk::launch_shuffle_blocks(d_shuf, out_off, n, elem, true, d_out, skip, size_hint, st);
    }
    if (skip != nullptr) {                                  // a stored block ignores the dictionary
        SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
        sqzk::launch_range_copy(d_in, in_off, d_out, out_off, out_off, stored, n, false, size_hint, st);
    }
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(d_out, out_off, n, crc, size_hint, st); }
}

// the device side of a frame decode, blocks [first, first + n_sel) into d_out (block `first` at its start)
int frame_decode_dev(const uint8_t* d_frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t first,
                     uint32_t n_sel, uint64_t sel_bytes, uint8_t* d_out, int32_t* d_err, int32_t* d_status,
                     uint8_t* scratch, uint64_t scratch_bytes, hipStream_t st, uint32_t version,
                     const uint8_t* d_dict = nullptr, uint32_t dict_bytes = 0, uint32_t want_bits = 0,
                     uint32_t elem = 0) {
    // elem: 2, 4 or 8 is the version-4 reader, and no other (never with a dictionary)
    const FrameScratch L = frame_scratch(n_sel, sel_bytes, 0, false, false, elem != 0);
    const uint64_t record = d_dict != nullptr || elem != 0 ? 8 : 0;    // a dictionary: the version-3 reader, and no other
    if (scratch_bytes < L.total || avail < 32 + 8 * (uint64_t)n + record) { return scratch_bytes < L.total ? EINVAL : E2BIG; }
    uint64_t* in_off = (uint64_t*)(scratch + L.in_off);
    uint64_t* out_off = (uint64_t*)(scratch + L.out_off);
    uint32_t* crc = (uint32_t*)(scratch + L.crc);
    uint32_t* stored = (uint32_t*)(scratch + L.stored);     // the same words as crc, one after the other (frame_scratch)
    uint64_t* idx_off = (uint64_t*)(scratch + L.misc);
    uint32_t* idx_crc = (uint32_t*)(scratch + L.misc + 16);
    uint64_t* spare = (uint64_t*)(scratch + L.misc + 32);
    // {0, 8 n}: the index as one range behind the header, written on the device (no host copy to wait for);
    // with the record of a version-3 frame {0, 8 n + 8}
    const uint64_t idx_bytes = 8 * (uint64_t)n + record;
    sqzk::launch_frame_plan(1, idx_bytes, idx_bytes, 0, idx_off, spare, st);
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(d_frame + 32, idx_off, 1, idx_crc, idx_bytes, st); }
    DictDev dd;
    if (d_dict != nullptr) {                                // the checksum of what the caller brought, for the open kernel
        uint64_t* dict_off = (uint64_t*)(scratch + L.misc + 64);        // [64,80) {0, D}, [96,112) spare, [128,132) its crc
        uint32_t* dict_crc = (uint32_t*)(scratch + L.misc + 128);
        sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, dict_off, dict_off + 4, st);
        { SpanGuard g(st, SQZ_HIP_K_CRC32);
          sqzk::launch_crc32_blocks(d_dict, dict_off, 1, dict_crc, dict_bytes, st); }
        SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
        sqzk::launch_frame_open_v3(d_frame, avail, n, content_bytes, first, n_sel, idx_crc, dict_bytes, dict_crc, in_off,
                                   out_off, stored, d_status, st, want_bits);
        dd.bytes = d_dict; dd.len = dict_bytes;
    } else if (elem != 0) {
        SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
        sqzk::launch_frame_open_v4(d_frame, avail, n, content_bytes, first, n_sel, idx_crc, elem, in_off, out_off, stored,
                                   d_status, st, want_bits);
    } else {
        SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
        sqzk::launch_frame_open_v2(d_frame, avail, n, content_bytes, first, n_sel, idx_crc, in_off, out_off, stored,
                                   d_status, st, want_bits);
    }
    // version: what a host copy of the header said, 0 when the caller has none (the device flavour).  Only a frame
    // known to be version 1 goes without the mask, and then without the copy launch
    const uint32_t* const skip = version == 1 ? nullptr : stored;
    if (n_sel > 0) {
        uint32_t* counts = (uint32_t*)(scratch + L.codec);
        uint32_t* tokens = (uint32_t*)(scratch + L.codec + align_up((uint64_t)n_sel * 4, 256));
        run_frame_decode(d_frame, in_off, out_off, n_sel, (sel_bytes + n_sel - 1) / n_sel, tokens, counts, d_out, d_err,
                         skip, stored, crc, dd, st, 0, elem != 0 ? scratch + L.shuf : nullptr, elem);
        sqzk::launch_frame_verify(d_frame, first, n_sel, crc, d_status, d_err, st);
    }
    return hip_errno(hipGetLastError());
}

// where the pieces of a ranged read's scratch lie: the decode's scratch for the covering blocks, the blocks
// themselves, the copy's work list
struct ReadScratch { FrameScratch dec; uint64_t blocks, plan, total; };
ReadScratch read_scratch(uint64_t n_sel, uint64_t sel_bytes, bool shuf = false) {
    ReadScratch R;
    R.dec = frame_scratch(n_sel, sel_bytes, 0, false, false, shuf);
    R.blocks = R.dec.total;
    R.plan = R.blocks + align_up(sel_bytes + 16, 256);
    R.total = R.plan + 256;
    return R;
}

// the device side of a ranged read: the covering blocks into the scratch (frame_decode_dev), then status and work
// list (frame_read_plan_kernel), then the range or nothing into d_out (range_copy_kernel).  The caller has checked
// the range against content_bytes and n against block_bits; length > 0
int frame_read_dev(const uint8_t* d_frame, uint64_t avail, uint32_t n, uint64_t content_bytes, uint32_t block_bits,
                   uint64_t offset, uint64_t length, uint8_t* d_out, int32_t* d_err, int32_t* d_status,
                   uint8_t* scratch, uint64_t scratch_bytes, hipStream_t st, const uint8_t* d_dict, uint32_t dict_bytes,
                   uint32_t elem = 0) {
    const uint64_t bb = 1ull << block_bits;
    const uint64_t first = offset >> block_bits, b_end = ((offset + length - 1) >> block_bits) + 1;
    const uint64_t n_sel = b_end - first;
    const uint64_t sel_bytes = (b_end * bb < content_bytes ? b_end * bb : content_bytes) - first * bb;
    const ReadScratch R = read_scratch(n_sel, sel_bytes, elem != 0);
    if (scratch_bytes < R.total) { return EINVAL; }
    uint8_t* const blocks = scratch + R.blocks;
    uint64_t* const plan = (uint64_t*)(scratch + R.plan);
    const int e = frame_decode_dev(d_frame, avail, n, content_bytes, (uint32_t)first, (uint32_t)n_sel, sel_bytes, blocks,
                                   d_err, d_status, scratch, R.dec.total, st, 0, d_dict, dict_bytes, block_bits, elem);
    if (e != 0) { return e; }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_frame_read_plan(d_err, (uint32_t)n_sel, offset - first * bb, length, plan, d_status, st); }
    { SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
      sqzk::launch_range_copy(blocks, plan, d_out, plan + 2, plan + 2, (const uint32_t*)(plan + 4), 1, false, length, st); }
    return hip_errno(hipGetLastError());
}

// host flavour of decode: blocks [b_first, b_end) of a frame that sqz_frame_info has checked WITH its index, in
// passes; sink(first block of the pass, blocks, their errnos, device pointer to their bytes, how many) takes what
// it wants of each pass with copies on st and returns an errno.  The device holds an image of the whole frame, of
// which only header, index and the streams of the blocks asked for are uploaded.
template <class Sink>
int frame_decode_host(Lane& c, hipStream_t st, const uint8_t* frame, const struct sqz_frame_info& fi,
                      uint64_t b_first, uint64_t b_end, Sink sink) {
    const uint64_t bb = fi.block_bytes, n = fi.n_blocks;
    // version 4: the record's elem_bytes (sqz_frame_info has checked it), and a pass's scratch holds its blocks shuffled
    const uint32_t elem = fi.version == 4 ? get_le32(frame + 32 + 8 * n) : 0u;
    std::vector<uint64_t> pre(n + 1);
    pre[0] = 0;
    for (uint64_t b = 0; b < n; b++) { pre[b + 1] = pre[b] + 8 * (uint64_t)frame_entry_words(frame, fi.version, b); }
    int e;
    if ((e = c.dense.reserve(fi.frame_bytes + 16)) || (e = c.misc.reserve(256))) { return e; }
    uint8_t* const d_frame = (uint8_t*)c.dense.p;
    HIP_TRY(hipMemcpyAsync(d_frame, frame, fi.payload_off, hipMemcpyHostToDevice, st));
    const uint64_t pass = frame_pass_blocks(bb);
    std::vector<int32_t> errs;
    for (uint64_t p0 = b_first; p0 < b_end; p0 += pass) {
        const uint64_t pn = b_end - p0 < pass ? b_end - p0 : pass;
        const uint64_t c0 = p0 * bb, c1 = (p0 + pn) * bb < fi.content_bytes ? (p0 + pn) * bb : fi.content_bytes;
        const FrameScratch L = frame_scratch(pn, c1 - c0, 0, false, false, elem != 0);
        if ((e = c.out.reserve(c1 - c0 + 16)) || (e = c.work_a.reserve(L.total)) || (e = c.err.reserve(pn * 4))) { return e; }
        if (pre[p0 + pn] > pre[p0]) {
            HIP_TRY(hipMemcpyAsync(d_frame + fi.payload_off + pre[p0], frame + fi.payload_off + pre[p0],
                                   pre[p0 + pn] - pre[p0], hipMemcpyHostToDevice, st));
        }
        if ((e = frame_decode_dev(d_frame, fi.frame_bytes, (uint32_t)n, fi.content_bytes, (uint32_t)p0, (uint32_t)pn,
                                  c1 - c0, (uint8_t*)c.out.p, (int32_t*)c.err.p, (int32_t*)c.misc.p,
                                  (uint8_t*)c.work_a.p, L.total, st, fi.version, nullptr, 0, 0, elem)) != 0) { return e; }
        errs.resize(pn);
        int32_t status = 0;
        HIP_TRY(hipMemcpyAsync(errs.data(), c.err.p, pn * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&status, c.misc.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (status != 0) { return status; }
        if ((e = sink(p0, pn, errs.data(), (const uint8_t*)c.out.p, c1 - c0)) != 0) { return e; }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

// Host flavour of decode for a version-3 frame (shared dictionary).  The host has checked header, index and
// record (sqz_frame_info), so the offsets and the stored mask of a pass are worked out here and uploaded with its
// streams, and the checksums come back to be compared here: the device-resident decode's open kernel, which
// refuses version 3, is not involved.  Same passes and the same sink as frame_decode_host, and the same kernels
// behind the offsets (run_frame_decode); what differs is where the offsets come from and where the checksums are
// compared, which is what version 3 in the device-resident flavour will fold back into one.
template <class Sink>
int frame_decode_host_dict(Lane& c, hipStream_t st, const uint8_t* frame, const struct sqz_frame_info& fi,
                           uint64_t b_first, uint64_t b_end, const DictDev& dd, Sink sink) {
    const uint64_t bb = fi.block_bytes, n = fi.n_blocks;
    std::vector<uint64_t> pre(n + 1);
    pre[0] = 0;
    for (uint64_t b = 0; b < n; b++) { pre[b + 1] = pre[b] + 8 * (uint64_t)frame_entry_words(frame, fi.version, b); }
    const uint64_t pass = frame_pass_blocks(bb);
    std::vector<uint64_t> io, oo;
    std::vector<uint32_t> mask, crc;
    std::vector<int32_t> errs;
    int e;
    for (uint64_t p0 = b_first; p0 < b_end; p0 += pass) {
        const uint64_t pn = b_end - p0 < pass ? b_end - p0 : pass;
        const uint64_t c0 = p0 * bb, c1 = (p0 + pn) * bb < fi.content_bytes ? (p0 + pn) * bb : fi.content_bytes;
        const uint64_t in_bytes = pre[p0 + pn] - pre[p0];
        io.resize(pn + 1); oo.resize(pn + 1); mask.resize(pn); crc.resize(pn); errs.resize(pn);
        bool any_stored = false;
        for (uint64_t k = 0; k <= pn; k++) {
            io[k] = pre[p0 + k] - pre[p0];
            oo[k] = ((p0 + k) * bb < fi.content_bytes ? (p0 + k) * bb : fi.content_bytes) - c0;
            if (k < pn) { mask[k] = frame_entry_stored(frame, fi.version, p0 + k) ? 1u : 0u; any_stored |= mask[k] != 0; }
        }
        if ((e = c.in.reserve(in_bytes + 16)) || (e = c.out.reserve(c1 - c0 + 16)) ||
            (e = c.in_off.reserve((pn + 1) * 8)) || (e = c.out_off.reserve((pn + 1) * 8)) ||
            (e = c.mask.reserve(pn * 4 + 4)) || (e = c.crc.reserve(pn * 4 + 4)) || (e = c.err.reserve(pn * 4)) ||
            (e = c.tokens.reserve((c1 - c0 + 64) * 4)) || (e = c.tok_count.reserve(pn * 4))) { return e; }
        if (in_bytes > 0) {
            HIP_TRY(hipMemcpyAsync(c.in.p, frame + fi.payload_off + pre[p0], in_bytes, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(c.in_off.p, io.data(), (pn + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c.out_off.p, oo.data(), (pn + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c.mask.p, mask.data(), pn * 4, hipMemcpyHostToDevice, st));
        const uint32_t* const skip = any_stored ? (const uint32_t*)c.mask.p : nullptr;
        const uint64_t hint = (c1 - c0 + pn - 1) / pn;
        run_frame_decode((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, (const uint64_t*)c.out_off.p, (uint32_t)pn,
                         hint, (uint32_t*)c.tokens.p, (uint32_t*)c.tok_count.p, (uint8_t*)c.out.p, (int32_t*)c.err.p,
                         skip, skip, (uint32_t*)c.crc.p, dd, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(errs.data(), c.err.p, pn * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(crc.data(), c.crc.p, pn * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t k = 0; k < pn; k++) {
            if (errs[k] == 0 && crc[k] != get_le32(frame + 32 + 8 * (p0 + k) + 4)) { errs[k] = EILSEQ; }
        }
        if ((e = sink(p0, pn, errs.data(), (const uint8_t*)c.out.p, c1 - c0)) != 0) { return e; }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

// a frame whose header, index AND extent the host has checked: what every host decode call starts with
int frame_check_host(const uint8_t* frame, uint64_t avail, struct sqz_frame_info* fi) {
    const int e = sqz_frame_info(frame, avail, fi);
    if (e != 0) { return e; }
    return avail < fi->payload_off ? E2BIG : 0;             // the index was not covered, so not checked
}

} // namespace

// =========================================================================
extern "C" {

const char* sqz_version(void) { return "sqz_amd 0.1 (gfx950; H0 semantics, H1 names)"; }

int sqz_hip_device_info(char* name, size_t name_cap, int* compute_units,
                        uint64_t* lds_bytes_per_cu) {
    Ctx& c = ctx();
    std::lock_guard<std::mutex> g(c.mu);
    const int e = probe_locked(c);
    if (e != 0) { return e; }
    if (name != NULL && name_cap > 0) { snprintf(name, name_cap, "%s", c.name); }
    if (compute_units != NULL) { *compute_units = c.cus; }
    if (lds_bytes_per_cu != NULL) { *lds_bytes_per_cu = c.lds; }
    return 0;
}

uint64_t sqz_bound(uint64_t bytes) { return (2 * bytes + 1024 + 7) & ~(uint64_t)7; }

int sqz_file_words(const uint8_t* in, uint64_t bytes, uint8_t* out) {
    if ((bytes & 7u) != 0 || (bytes != 0 && (in == NULL || out == NULL))) { return EINVAL; }
    for (uint64_t k = 0; k < bytes; k += 8) {
        uint64_t w = 0;                                   // the word's value: stream bytes are MSB first
        for (int j = 0; j < 8; j++) { w = (w << 8) | in[k + j]; }
        memcpy(out + k, &w, 8);                           // what fwrite(&b64, 8, 1, f) puts in the file
    }
    return 0;
}

void sqz_init(struct sqz* s) {
    if (s == NULL) { return; }
    memset(s, 0, sizeof(*s));
    s->device = -1;
}

void sqz_write_header(struct bitstream* bs, uint64_t bytes) { host_put_bits(bs, bytes, 64); }

void sqz_read_header(struct bitstream* bs, uint64_t* bytes) {
    const uint64_t b = host_get_bits(bs, 64);
    if (bs->error == 0 && bytes != NULL) { *bytes = b; }
}

void sqz_write_header_h0(struct bitstream* bs, uint64_t bytes, uint8_t win_bits) {
    if (win_bits < sqz_min_win_bits || win_bits > sqz_max_win_bits) {   // squeeze.h:257-258
        bs->error = EINVAL;
    } else {
        host_put_bits(bs, bytes, 64);
        host_put_bits(bs, win_bits, 8);
    }
}

void sqz_read_header_h0(struct bitstream* bs, uint64_t* bytes, uint8_t* win_bits) {
    const uint64_t b = host_get_bits(bs, 64);
    const uint64_t w = host_get_bits(bs, 8);
    if (bs->error == 0) {
        if (w < sqz_min_win_bits || w > sqz_max_win_bits) {             // squeeze.h:449-450
            bs->error = EINVAL;
        } else {
            if (bytes != NULL) { *bytes = b; }
            if (win_bits != NULL) { *win_bits = (uint8_t)w; }
        }
    }
}

void sqz_compress(struct sqz* s, struct bitstream* bs,
                  const uint8_t* data, size_t bytes, uint32_t window) {
    if (s == NULL || bs == NULL) { return; }
    s->bs = bs;                                          // squeeze.h:332
    if (s->error != 0) { return; }                       // sticky: squeeze.h:337
    if (bs->error != 0) { s->error = bs->error; return; } // squeeze.h:226-227
    const bool by_callback = writer_is_callback(bs);
    if (!window_ok(window) || (!by_callback && !writer_is_memory(bs)) ||
        (bytes > 0 && data == NULL) || bytes > kMaxStream || (!by_callback && bs->bytes > bs->capacity) ||
        bs->bits < 0 || bs->bits > 63) {
        s->error = EINVAL;
        return;
    }
    // callback mode: the stream lands in a buffer of ours and is handed over word by word below
    std::vector<uint8_t> own;
    uint8_t* dst = by_callback ? nullptr : bs->data + bs->bytes;
    uint64_t room = by_callback ? 0 : bs->capacity - bs->bytes;
    if (by_callback) {
        room = sqz_bound(bytes) + 16;
        own.resize(room);
        dst = own.data();
    }
    const uint64_t in_off[2] = {0, (uint64_t)bytes};
    const uint64_t out_off[2] = {0, room};
    uint64_t produced = 0;
    int32_t err = 0;
    {
        int e = device_ready();
        if (e != 0) { s->error = e; return; }
        // the device writes into a staging slab; it lands behind the header bytes
        LaneLease lease;
        e = encode_host(*lease.lane, lease.stream(s->stream), data, in_off, 1, window, dst, out_off, &produced,
                        &err, bs->b64, bs->bits, &s->tokens);
        if (e != 0) { s->error = e; return; }
    }
    bs->b64 = 0;
    bs->bits = 0;
    if (by_callback) {                                   // bitstream.h:44-48, one call per word
        for (uint64_t k = 0; k + 8 <= produced && bs->error == 0; k += 8) {
            bs->b64 = load_be64(dst + k);
            bs->error = bs->output(bs);
            if (bs->error == 0) { bs->bytes += 8; }
            bs->b64 = 0;
        }
        if (err == 0) { err = bs->error; }               // squeeze.h:226-236 mirrors the stream's error
    } else {
        bs->bytes += produced;
        if (err == E2BIG) { bs->error = E2BIG; }
    }
    s->error = err;
}

// leave the reader where the reference's would be after the symbol that ended at `end_bit`
// of buf[0 .. limit): bitstream.h:65-93 (the last fetched word, shifted by what was consumed)
static void park_reader(bitstream* bs, const uint8_t* buf, uint64_t limit, uint64_t end_bit,
                        uint64_t* words_out) {
    const uint64_t words = (end_bit + 63) / 64;
    bs->bits = (int32_t)(words * 64 - end_bit);
    bs->b64 = 0;
    if (bs->bits > 0 && words * 8 <= limit) { bs->b64 = load_be64(buf + (words - 1) * 8) << (64 - bs->bits); }
    *words_out = words;
}

static void decompress_by_callback(struct sqz* s, struct bitstream* bs, uint8_t* data, size_t bytes) {
    // What the header reader left: `bits` unread bits at the top of b64.  They become word 0 of
    // our buffer (the bits in front of them are gone; the decoder starts behind them).
    std::vector<uint8_t> buf;
    uint64_t start_bit = 0;
    if (bs->bits > 0) {
        buf.resize(8);
        store_be64(buf.data(), bs->b64 >> (64 - bs->bits));
        start_bit = 64 - (uint64_t)bs->bits;
    }
    const uint64_t head_words = buf.size() / 8;
    const uint64_t most_words = head_words + (sqz_bound(bytes) + 16) / 8 + 2;   // no stream of `bytes` bytes is longer
    // The reference pulls one word when its bit reader runs dry (bitstream.h:81-85); a device decode wants
    // its input up front and a word cannot be handed back, so the pull runs AHEAD of the decoder: 4 words,
    // then twice as many whenever the decoder ran dry.  Words pulled <= max(4, 2 x the words the stream
    // holds) whatever its compression ratio; every retry decodes again from the stream's start.
    uint64_t want_words = head_words + 4;
    int src_error = 0;
    bool dry = false;
    for (;;) {
        if (want_words > most_words) { want_words = most_words; }
        while (buf.size() / 8 < want_words && !dry) {        // bitstream.h:81-85
            bs->b64 = 0;
            const int e = bs->input(bs);
            if (e != 0) { src_error = e; dry = true; break; }
            const size_t at = buf.size();
            buf.resize(at + 8);
            store_be64(buf.data() + at, bs->b64);
        }
        const uint64_t limit = buf.size();
        const uint64_t in_off[2] = {0, limit};
        const uint64_t out_off[2] = {0, (uint64_t)bytes};
        int32_t err = 0;
        uint64_t end_bit = 0;
        {
            int e = device_ready();
            if (e == 0) {
                LaneLease lease;
                e = decode_host(*lease.lane, lease.stream(s->stream), buf.data(), in_off, 1, data, out_off, &err,
                                start_bit, &end_bit);
            }
            if (e != 0) { s->error = e; return; }
        }
        if (err == E2BIG && !dry && limit / 8 < most_words) {   // ran out of words: pull more and decode again
            want_words = head_words + 2 * (limit / 8 - head_words);
            continue;
        }
        uint64_t words = 0;
        park_reader(bs, buf.data(), limit, end_bit, &words);
        if (words > limit / 8) { words = limit / 8; }
        bs->read += 8 * (words - head_words);                // what the reference's reader would have fetched
        if (err == E2BIG) {                                  // the source ended before the stream did
            bs->error = src_error != 0 ? src_error : E2BIG;
            err = bs->error;
        }
        s->error = err;
        return;
    }
}

void sqz_decompress(struct sqz* s, struct bitstream* bs, uint8_t* data, size_t bytes) {
    if (s == NULL || bs == NULL) { return; }
    s->bs = bs;                                          // squeeze.h:504
    if (s->error != 0) { return; }
    if (bs->error != 0) { s->error = bs->error; return; }
    if ((bytes > 0 && data == NULL) || bytes > kMaxStream || bs->bits < 0 || bs->bits > 63) {
        s->error = EINVAL;
        return;
    }
    if (reader_is_callback(bs)) {
        if (bytes != 0) { decompress_by_callback(s, bs, data, bytes); }
        return;
    }
    const uint64_t limit = reader_limit(bs);
    if (bs->data == NULL || bs->read > limit || (uint64_t)bs->bits > bs->read * 8) {
        s->error = EINVAL;
        return;
    }
    if (bytes == 0) { return; }
    const uint64_t start_bit = bs->read * 8 - (uint64_t)bs->bits;
    const uint64_t in_off[2] = {0, limit};
    const uint64_t out_off[2] = {0, (uint64_t)bytes};
    int32_t err = 0;
    uint64_t end_bit = 0;
    {
        int e = device_ready();
        if (e == 0) {
            LaneLease lease;
            e = decode_host(*lease.lane, lease.stream(s->stream), bs->data, in_off, 1, data, out_off, &err,
                            start_bit, &end_bit);
        }
        if (e != 0) { s->error = e; return; }
    }
    uint64_t words = 0;
    park_reader(bs, bs->data, limit, end_bit, &words);
    bs->read = words * 8 <= limit ? words * 8 : limit;
    if (err == E2BIG) { bs->error = E2BIG; }
    s->error = err;
}

// ------------------------------------------------------------------ vtable
static squeeze_type* vt_alloc(uint8_t map_bits) {
    if (map_bits != 0) { return NULL; }
    squeeze_type* s = (squeeze_type*)calloc(1, sizeof(squeeze_type));
    if (s != NULL) { sqz_init(s); }
    return s;
}
static int vt_init_with(squeeze_type* s, void* memory, size_t size, uint8_t map_bits) {
    // squeeze.h:191-199: size == squeeze_sizeof(map_bits).  The codec state lives on the device, so the
    // caller's block only has to hold the struct; a block sized for the reference's trees is accepted too.
    if (map_bits != 0 || memory == NULL || s != memory || size < squeeze_sizeof(0)) { return EINVAL; }
    sqz_init(s);
    return 0;
}
static void vt_compress(squeeze_type* s, bitstream* bs, const uint8_t* data, size_t bytes,
                        uint16_t window) {
    sqz_compress(s, bs, data, bytes, window);
}
static void vt_free(squeeze_type* s) { free(s); }

squeeze_interface squeeze = {
    vt_alloc, vt_init_with, sqz_write_header_h0, vt_compress,
    sqz_read_header_h0, sqz_decompress, vt_free
};

// ------------------------------------------------------------------ batch, host
int sqz_encode_blocks(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint32_t window,
                      uint8_t* out, const uint64_t* out_off, uint64_t* out_bytes, int32_t* err) {
    return sqz_encode_blocks_parse(in, in_off, n, window, SQZ_PARSE_GREEDY, out, out_off, out_bytes, err);
}

int sqz_encode_blocks_parse(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint32_t window, uint32_t parse,
                            uint8_t* out, const uint64_t* out_off, uint64_t* out_bytes, int32_t* err) {
    if (!parse_ok(parse)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (in_off == NULL || out_off == NULL || out == NULL || out_bytes == NULL || err == NULL ||
        !window_ok(window)) { return EINVAL; }
    if (check_offsets(in_off, n, false) != 0 || check_offsets(out_off, n, true) != 0) { return EINVAL; }
    if (in == NULL && in_off[n] != in_off[0]) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    LaneLease lease;
    return encode_host(*lease.lane, lease.stream(nullptr), in, in_off, n, window, out, out_off, out_bytes, err,
                       0, 0, nullptr, parse);
}

int sqz_decode_blocks(const uint8_t* in, const uint64_t* in_off, uint32_t n,
                      uint8_t* out, const uint64_t* out_off, int32_t* err) {
    if (n == 0) { return 0; }
    if (in == NULL || in_off == NULL || out_off == NULL || err == NULL) { return EINVAL; }
    if (check_offsets(in_off, n, true) != 0 || check_offsets(out_off, n, false) != 0) { return EINVAL; }
    if (out == NULL && out_off[n] != out_off[0]) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    LaneLease lease;
    return decode_host(*lease.lane, lease.stream(nullptr), in, in_off, n, out, out_off, err, 0, nullptr);
}

int sqz_encode_blocks_dict(const uint8_t* in, const uint64_t* in_off, uint32_t n, uint32_t window, uint32_t parse,
                           const uint8_t* dict, uint64_t dict_bytes, uint8_t* out, const uint64_t* out_off,
                           uint64_t* out_bytes, int32_t* err) {
    if (!parse_ok(parse) || !window_ok(window) || !dict_ok(dict, dict_bytes, window)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (in_off == NULL || out_off == NULL || out == NULL || out_bytes == NULL || err == NULL) { return EINVAL; }
    if (check_offsets(in_off, n, false) != 0 || check_offsets(out_off, n, true) != 0) { return EINVAL; }
    if (in == NULL && in_off[n] != in_off[0]) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    LaneLease lease;
    return encode_host(*lease.lane, lease.stream(nullptr), in, in_off, n, window, out, out_off, out_bytes, err,
                       0, 0, nullptr, parse, dict, (uint32_t)dict_bytes);
}

int sqz_decode_blocks_dict(const uint8_t* in, const uint64_t* in_off, uint32_t n, const uint8_t* dict,
                           uint64_t dict_bytes, uint8_t* out, const uint64_t* out_off, int32_t* err) {
    if (!dict_ok(dict, dict_bytes, (uint32_t)sqzk_max_window)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (in == NULL || in_off == NULL || out_off == NULL || err == NULL) { return EINVAL; }
    if (check_offsets(in_off, n, true) != 0 || check_offsets(out_off, n, false) != 0) { return EINVAL; }
    if (out == NULL && out_off[n] != out_off[0]) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    LaneLease lease;
    return decode_host(*lease.lane, lease.stream(nullptr), in, in_off, n, out, out_off, err, 0, nullptr, dict,
                       (uint32_t)dict_bytes);
}

// ------------------------------------------------------------------ batch, device
uint64_t sqz_hip_encode_scratch_bytes_dict(uint32_t n, uint64_t total_in_bytes, uint64_t dict_bytes) {
    return dict_index_bytes(dict_bytes) + sqz_hip_encode_scratch_bytes(n, total_in_bytes);
}

uint64_t sqz_hip_encode_scratch_bytes(uint32_t n, uint64_t total_in_bytes) {
    // token counts + two uint32 slots per input byte: sorted positions, later the token words / the sort's
    // second buffer, later the match table
    return align_up((uint64_t)n * 4, 256) + 2 * (total_in_bytes + 64) * 4;
}

int sqz_hip_lz77_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                        uint32_t* d_tokens, uint32_t* d_token_count, void* stream) {
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_tokens == NULL || d_token_count == NULL ||
        !window_ok(window)) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    run_stage1(0, (const uint8_t*)d_in, d_in_off, n, window, d_tokens, d_token_count,
               nullptr, nullptr, 0, ~0ull /* d_tokens: one slot per input byte, by contract */,
               (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

int sqz_hip_lz77_blocks_ex(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                           uint32_t* d_tokens, uint32_t* d_token_count, int finder,
                           void* d_work, uint64_t work_bytes, void* stream) {
    return sqz_hip_lz77_blocks_parse(d_in, d_in_off, n, window, d_tokens, d_token_count, finder, SQZ_PARSE_GREEDY,
                                     d_work, work_bytes, stream);
}

int sqz_hip_lz77_blocks_parse(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                              uint32_t* d_tokens, uint32_t* d_token_count, int finder, uint32_t parse,
                              void* d_work, uint64_t work_bytes, void* stream) {
    if (!parse_ok(parse) || (parse == SQZ_PARSE_LAZY && finder != 1)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_tokens == NULL || d_token_count == NULL ||
        !window_ok(window) || (finder != 0 && finder != 1)) { return EINVAL; }
    if (finder == 1 && (d_work == NULL || work_bytes < 8 * 64)) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    // work = two arrays of work_bytes/8 uint32 slots (sorted positions, match table)
    const uint64_t slots = work_bytes / 8;
    uint32_t* wa = (uint32_t*)d_work;
    uint32_t* wm = wa != nullptr ? wa + slots : nullptr;
    run_stage1(finder, (const uint8_t*)d_in, d_in_off, n, window, d_tokens, d_token_count,
               finder == 1 ? wa : nullptr, finder == 1 ? wm : nullptr,
               slots / (n > 0 ? n : 1), finder == 1 ? slots : ~0ull, (hipStream_t)stream, parse);
    return hip_errno(hipGetLastError());
}

int sqz_hip_lz77_blocks_dict(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                             uint32_t* d_tokens, uint32_t* d_token_count, int finder, uint32_t parse,
                             const void* d_dict, uint64_t dict_bytes, void* d_work, uint64_t work_bytes, void* stream) {
    // the scan finder has no match table to merge into
    if (!parse_ok(parse) || finder != 1 || !window_ok(window) || !dict_ok(d_dict, dict_bytes, window)) { return EINVAL; }
    const uint64_t head = dict_index_bytes(dict_bytes);
    if (d_work == NULL || ((uintptr_t)d_work & 15u) != 0 || work_bytes < head + 8 * 64) { return EINVAL; }
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_tokens == NULL || d_token_count == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    const DictDev dd = run_dict_index((const uint8_t*)d_dict, (uint32_t)dict_bytes, (uint8_t*)d_work, (hipStream_t)stream);
    const uint64_t slots = (work_bytes - head) / 8;
    uint32_t* wa = (uint32_t*)((uint8_t*)d_work + head);
    run_stage1(1, (const uint8_t*)d_in, d_in_off, n, window, d_tokens, d_token_count, wa, wa + slots,
               slots / n, slots, (hipStream_t)stream, parse, &dd);
    return hip_errno(hipGetLastError());
}

int sqz_hip_huffman_blocks(const uint32_t* d_tokens, const uint64_t* d_in_off,
                           const uint32_t* d_token_count, uint32_t n, void* d_out,
                           const uint64_t* d_out_off, uint64_t* d_out_bytes, int32_t* d_err,
                           void* stream) {
    if (n == 0) { return 0; }
    if (d_tokens == NULL || d_in_off == NULL || d_token_count == NULL || d_out == NULL ||
        d_out_off == NULL || d_out_bytes == NULL || d_err == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    SpanGuard g((hipStream_t)stream, SQZ_HIP_K_HUFFMAN_EMIT);
    sqzk::launch_huffman_emit(d_tokens, d_in_off, d_token_count, (uint8_t*)d_out, d_out_off,
                             d_out_bytes, d_err, n, 0, 0, nullptr, (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

int sqz_hip_encode_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                          void* d_out, const uint64_t* d_out_off, uint64_t* d_out_bytes,
                          int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return sqz_hip_encode_blocks_stats(d_in, d_in_off, n, window, d_out, d_out_off, d_out_bytes, d_err,
                                       d_scratch, scratch_bytes, NULL, stream);
}

static int encode_blocks_dev(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window, uint32_t parse,
                             void* d_out, const uint64_t* d_out_off, uint64_t* d_out_bytes, int32_t* d_err,
                             void* d_scratch, uint64_t scratch_bytes, sqz_block_stats* d_stats, void* stream);

int sqz_hip_encode_blocks_parse(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                                uint32_t parse, void* d_out, const uint64_t* d_out_off, uint64_t* d_out_bytes,
                                int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!parse_ok(parse)) { return EINVAL; }
    return encode_blocks_dev(d_in, d_in_off, n, window, parse, d_out, d_out_off, d_out_bytes, d_err,
                             d_scratch, scratch_bytes, NULL, stream);
}

double sqz_stats_entropy(const uint32_t* freq, uint32_t n) {          // huffman.h:237-249
    if (freq == NULL) { return 0.0; }
    double total = 0.0, e = 0.0;
    for (uint32_t i = 0; i < n; i++) { total += (double)freq[i]; }
    for (uint32_t i = 0; i < n; i++) {
        if (freq[i] > 0) {
            const double p = (double)freq[i] / total;
            e += p * log2(p);
        }
    }
    return -e;
}

int sqz_hip_encode_blocks_stats(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window,
                                void* d_out, const uint64_t* d_out_off, uint64_t* d_out_bytes,
                                int32_t* d_err, void* d_scratch, uint64_t scratch_bytes,
                                sqz_block_stats* d_stats, void* stream) {
    return encode_blocks_dev(d_in, d_in_off, n, window, SQZ_PARSE_GREEDY, d_out, d_out_off, d_out_bytes, d_err,
                             d_scratch, scratch_bytes, d_stats, stream);
}

static int encode_blocks_dev(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window, uint32_t parse,
                             void* d_out, const uint64_t* d_out_off, uint64_t* d_out_bytes, int32_t* d_err,
                             void* d_scratch, uint64_t scratch_bytes, sqz_block_stats* d_stats, void* stream) {
    if (n == 0) { return 0; }
    if (d_scratch == NULL || scratch_bytes < sqz_hip_encode_scratch_bytes(n, 0)) { return EINVAL; }
    if (d_in == NULL || d_in_off == NULL || d_out == NULL || d_out_off == NULL ||
        d_out_bytes == NULL || d_err == NULL || !window_ok(window)) { return EINVAL; }
    int e = device_ready();
    if (e != 0) { return e; }
    const uint64_t head = align_up((uint64_t)n * 4, 256);
    // The offsets live on the device, so whether in_off[n] fits the scratch cannot be checked here
    // without a round trip: the kernels get `slots` and refuse (EINVAL, that block only) any
    // block whose in_off[b+1] lies beyond it.  Offsets are absolute slot indices: in_off[0]
    // need not be 0, but the arrays are addressed by them.
    const uint64_t slots = (scratch_bytes - head) / 8;     // >= total_in_bytes + 64 by contract
    uint32_t* counts = (uint32_t*)d_scratch;
    uint32_t* tokens = (uint32_t*)((uint8_t*)d_scratch + head);
    uint32_t* work_a = tokens;                             // sorted positions first, the token words afterwards
    uint32_t* work_m = work_a + slots;
    run_encode(finder_for(parse), (const uint8_t*)d_in, d_in_off, n, window, tokens, counts,
               work_a, work_m, slots / n, (uint8_t*)d_out, d_out_off, d_out_bytes, d_err, 0, 0,
               slots, d_stats, (hipStream_t)stream, parse);
    return hip_errno(hipGetLastError());
}

int sqz_hip_encode_blocks_dict(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t window, uint32_t parse,
                               const void* d_dict, uint64_t dict_bytes, void* d_out, const uint64_t* d_out_off,
                               uint64_t* d_out_bytes, int32_t* d_err, void* d_scratch, uint64_t scratch_bytes,
                               void* stream) {
    if (!parse_ok(parse) || !window_ok(window) || !dict_ok(d_dict, dict_bytes, window)) { return EINVAL; }
    if (d_scratch == NULL || ((uintptr_t)d_scratch & 15u) != 0 ||
        scratch_bytes < sqz_hip_encode_scratch_bytes_dict(n, 0, dict_bytes)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_out == NULL || d_out_off == NULL || d_out_bytes == NULL ||
        d_err == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    // the dictionary's index first, then the scratch of sqz_hip_encode_blocks
    const uint64_t idx = dict_index_bytes(dict_bytes);
    const DictDev dd = run_dict_index((const uint8_t*)d_dict, (uint32_t)dict_bytes, (uint8_t*)d_scratch, (hipStream_t)stream);
    uint8_t* const rest = (uint8_t*)d_scratch + idx;
    const uint64_t head = align_up((uint64_t)n * 4, 256);
    const uint64_t slots = (scratch_bytes - idx - head) / 8;
    uint32_t* counts = (uint32_t*)rest;
    uint32_t* tokens = (uint32_t*)(rest + head);
    run_encode(1, (const uint8_t*)d_in, d_in_off, n, window, tokens, counts, tokens, tokens + slots, slots / n,
               (uint8_t*)d_out, d_out_off, d_out_bytes, d_err, 0, 0, slots, nullptr, (hipStream_t)stream, parse, &dd);
    return hip_errno(hipGetLastError());
}

int sqz_hip_decode_blocks_dict(const void* d_in, const uint64_t* d_in_off, uint32_t n, const void* d_dict,
                               uint64_t dict_bytes, void* d_out, const uint64_t* d_out_off, int32_t* d_err,
                               void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!dict_ok(d_dict, dict_bytes, (uint32_t)sqzk_max_window)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_out == NULL || d_out_off == NULL || d_err == NULL ||
        d_scratch == NULL || scratch_bytes < sqz_hip_decode_scratch_bytes(n, 0)) {
        return EINVAL;
    }
    const int e = device_ready();
    if (e != 0) { return e; }
    uint32_t* counts = (uint32_t*)d_scratch;
    uint32_t* tokens = (uint32_t*)((uint8_t*)d_scratch + align_up((uint64_t)n * 4, 256));
    { SpanGuard g((hipStream_t)stream, SQZ_HIP_K_ENTROPY_DECODE);
      sqzk::launch_entropy_decode((const uint8_t*)d_in, d_in_off, d_out_off, tokens, counts, d_err,
                                  nullptr, n, 0, decode_waves_for(n), (hipStream_t)stream, nullptr, (uint32_t)dict_bytes); }
    { SpanGuard g((hipStream_t)stream, SQZ_HIP_K_LZ_EXPAND);
      sqzk::launch_lz_expand(tokens, counts, (uint8_t*)d_out, d_out_off, n, (hipStream_t)stream, nullptr,
                             (const uint8_t*)d_dict, (uint32_t)dict_bytes); }
    return hip_errno(hipGetLastError());
}

uint64_t sqz_hip_decode_scratch_bytes(uint32_t n, uint64_t total_out_bytes) {
    return align_up((uint64_t)n * 4, 256) + (total_out_bytes + 64) * 4;
}

int sqz_hip_decode_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n, void* d_out,
                          const uint64_t* d_out_off, int32_t* d_err,
                          void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_out == NULL || d_out_off == NULL || d_err == NULL ||
        d_scratch == NULL || scratch_bytes < sqz_hip_decode_scratch_bytes(n, 0)) {
        return EINVAL;
    }
    const int e = device_ready();
    if (e != 0) { return e; }
    uint32_t* counts = (uint32_t*)d_scratch;
    uint32_t* tokens = (uint32_t*)((uint8_t*)d_scratch + align_up((uint64_t)n * 4, 256));
    { SpanGuard g((hipStream_t)stream, SQZ_HIP_K_ENTROPY_DECODE);
      sqzk::launch_entropy_decode((const uint8_t*)d_in, d_in_off, d_out_off, tokens, counts, d_err,
                                  nullptr, n, 0, decode_waves_for(n), (hipStream_t)stream); }
    { SpanGuard g((hipStream_t)stream, SQZ_HIP_K_LZ_EXPAND);
      sqzk::launch_lz_expand(tokens, counts, (uint8_t*)d_out, d_out_off, n, (hipStream_t)stream); }
    return hip_errno(hipGetLastError());
}

int sqz_hip_debug_tree(const int32_t* d_symbols, uint32_t count, int which, int batch,
                       uint32_t* d_dump, void* stream) {
    if (d_symbols == NULL || d_dump == NULL || ((which & 0xFF) != 0 && (which & 0xFF) != 1)) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    sqzk::launch_tree_debug(d_symbols, count, which, batch, d_dump, (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

int sqz_hip_pack_blocks(const void* d_slabs, const uint64_t* d_slab_off, const uint64_t* d_bytes,
                        uint32_t n, void* d_dense, const uint64_t* d_dense_off,
                        uint64_t avg_bytes, void* stream) {
    if (n == 0) { return 0; }
    if (d_slabs == NULL || d_slab_off == NULL || d_bytes == NULL || d_dense == NULL ||
        d_dense_off == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    sqzk::launch_compact_blocks((const uint8_t*)d_slabs, d_slab_off, d_bytes, n, (uint8_t*)d_dense,
                                d_dense_off, avg_bytes, (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

void sqz_hip_set_finder(int finder) { g_finder.store(finder == 0 ? 0 : 1); }
int  sqz_hip_get_finder(void) { return finder_default(); }

// ------------------------------------------------------------------ R-era API (include/sqz/sqz_rc.h)
uint64_t sqz_rc_bound(uint64_t bytes) { return 2 * bytes + 64; }

void sqz_rc_init(struct sqz_rc* s, struct sqz_rc_map_entry entry[], size_t n) {       // src/sqz.c:550-565
    (void)entry; (void)n;                     // HEAD disables its map inside sqz_compress (src/sqz.c:591)
    if (s == NULL) { return; }
    s->rc.low = 0;                            // rc_init :485-490 (write / read / that are the caller's)
    s->rc.range = ~0ull;
    s->rc.code = 0;
    s->rc.error = 0;
    memset(s->reserved, 0, sizeof(s->reserved));
}

int sqz_hip_rc_encode_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n, void* d_out,
                             const uint64_t* d_out_off, uint64_t* d_out_bytes, int32_t* d_err, void* stream) {
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_out == NULL || d_out_off == NULL || d_out_bytes == NULL ||
        d_err == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    SpanGuard g((hipStream_t)stream, SQZ_HIP_K_RC_ENCODE);
    sqzk::launch_rc_encode((const uint8_t*)d_in, d_in_off, (uint8_t*)d_out, d_out_off, d_out_bytes, d_err, n,
                           (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

int sqz_hip_rc_decode_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n, void* d_out,
                             const uint64_t* d_out_off, uint64_t* d_out_bytes, uint64_t* d_consumed,
                             int32_t* d_err, void* stream) {
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_out == NULL || d_out_off == NULL || d_out_bytes == NULL ||
        d_err == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    SpanGuard g((hipStream_t)stream, SQZ_HIP_K_RC_DECODE);
    sqzk::launch_rc_decode((const uint8_t*)d_in, d_in_off, (uint8_t*)d_out, d_out_off, d_out_bytes, d_consumed,
                           d_err, n, 0, (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

// one stream through the device, host buffers; returns a HIP-side errno (0 = the kernel ran)
static int rc_run_host(bool decode, const uint8_t* in, uint64_t in_bytes, uint8_t* out, uint64_t out_cap,
                       uint64_t* produced, uint64_t* consumed, int32_t* err, int dry_error) {
    int e = device_ready();
    if (e != 0) { return e; }
    LaneLease lease;
    Lane& c = *lease.lane;
    hipStream_t st = lease.stream(nullptr);
    if ((e = c.in.reserve(in_bytes + 16)) || (e = c.out.reserve(out_cap + 16)) || (e = c.in_off.reserve(16)) ||
        (e = c.out_off.reserve(16)) || (e = c.out_bytes.reserve(16)) || (e = c.err.reserve(8))) { return e; }
    const uint64_t io[2] = {0, in_bytes}, oo[2] = {0, out_cap};
    if (in_bytes > 0) { HIP_TRY(hipMemcpyAsync(c.in.p, in, in_bytes, hipMemcpyHostToDevice, st)); }
    HIP_TRY(hipMemcpyAsync(c.in_off.p, io, 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c.out_off.p, oo, 16, hipMemcpyHostToDevice, st));
    uint64_t* d_sizes = (uint64_t*)c.out_bytes.p;               // [0] produced, [1] consumed
    if (decode) {
        sqzk::launch_rc_decode((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, (uint8_t*)c.out.p,
                               (const uint64_t*)c.out_off.p, d_sizes, d_sizes + 1, (int32_t*)c.err.p, 1, dry_error, st);
    } else {
        sqzk::launch_rc_encode((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, (uint8_t*)c.out.p,
                               (const uint64_t*)c.out_off.p, d_sizes, (int32_t*)c.err.p, 1, st);
    }
    HIP_TRY(hipGetLastError());
    uint64_t sizes[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(sizes, d_sizes, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(err, c.err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t got = sizes[0] < out_cap ? sizes[0] : out_cap;
    if (got > 0) {
        HIP_TRY(hipMemcpyAsync(out, c.out.p, got, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *produced = sizes[0];
    if (consumed != NULL) { *consumed = decode ? sizes[1] : 0; }
    return 0;
}

void sqz_rc_compress(struct sqz_rc* s, const void* d, size_t b, uint32_t window) {   // src/sqz.c:590-791
    (void)window;                               // unused at HEAD but for an assert (:656)
    if (s == NULL || s->rc.error != 0) { return; }
    if ((b > 0 && d == NULL) || s->rc.write == NULL || b > kMaxStream) { s->rc.error = EINVAL; return; }
    std::vector<uint8_t> buf(sqz_rc_bound(b));
    uint64_t produced = 0;
    int32_t err = 0;
    const int e = rc_run_host(false, (const uint8_t*)d, b, buf.data(), buf.size(), &produced, NULL, &err, 0);
    if (e != 0) { s->rc.error = e; return; }
    if (err != 0) { s->rc.error = err; return; }
    for (uint64_t k = 0; k < produced && s->rc.error == 0; k++) { s->rc.write(&s->rc, buf[k]); }   // rc_emit :474-476
}

uint64_t sqz_rc_decompress(struct sqz_rc* s, void* data, size_t bytes) {               // src/sqz.c:793-839
    if (s == NULL || s->rc.error != 0) { return 0; }
    if ((bytes > 0 && data == NULL) || s->rc.read == NULL || bytes > kMaxStream) { s->rc.error = EINVAL; return 0; }
    std::vector<uint8_t> in;
    const uint64_t most = sqz_rc_bound(bytes) + 64;             // no stream of `bytes` literals is longer
    // The reference reads a byte when its decoder needs one (rc_consume :499-500); a device decode wants its
    // input up front, so the pull runs AHEAD of the decoder: 64 bytes, then twice as much each time the decoder
    // ran dry, decoding again from the start.  OVER-READ BOUND: at most max(64, 2 x the bytes the decoder
    // consumes) are pulled through rc.read (include/sqz/sqz_rc.h).
    uint64_t want = 64;
    bool dry = false;
    int src_error = 0;
    for (;;) {
        if (want > most) { want = most; }
        while (in.size() < want && !dry) {                      // rc_consume :499-500, ahead of the decoder
            const uint8_t v = s->rc.read(&s->rc);
            if (s->rc.error != 0) { src_error = s->rc.error; s->rc.error = 0; dry = true; break; }
            in.push_back(v);
        }
        uint64_t produced = 0, consumed = 0;
        int32_t err = 0;
        // a source that ended with an error: the decoder's first read past it sets that error, as the
        // reference's read callback does (test.c:112-121), and the loop ends where the reference's would
        const int e = rc_run_host(true, in.data(), in.size(), (uint8_t*)data, bytes, &produced, &consumed, &err,
                                  dry ? src_error : 0);
        if (e != 0) { s->rc.error = e; return 0; }
        if (consumed > in.size() && !dry && in.size() < most) { // ran past what was pulled: pull more, decode again
            want = 2 * in.size();
            continue;
        }
        s->rc.error = err;
        return produced < bytes ? produced : bytes;
    }
}

// ------------------------------------------------------------------ SQZF frames
uint64_t sqz_frame_bound(uint64_t content_bytes, uint32_t block_bits) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits) { return 0; }
    const uint64_t bb = 1ull << block_bits, full = content_bytes >> block_bits, tail = content_bytes & (bb - 1);
    return frame_payload_off(full + (tail != 0 ? 1 : 0)) + full * sqz_bound(bb) + (tail != 0 ? sqz_bound(tail) : 0);
}

int sqz_frame_info(const uint8_t* frame, uint64_t avail, struct sqz_frame_info* out) {
    if (frame == NULL || out == NULL) { return EINVAL; }
    if (avail < 32) { return E2BIG; }
    const uint32_t win_bits = frame[5], block_bits = frame[6];
    // version 1 has no flags; version 2 has at least one, and only known ones; version 3 iff SQZ_FRAME_DICT;
    // version 4 iff SQZ_FRAME_SHUFFLE (so never both)
    const uint32_t version = frame[4], flags = frame[7];
    const bool version_ok = (version == 1 && flags == 0) || (version == 2 && flags == (uint32_t)SQZ_FRAME_STORED) ||
                            (version == 3 && (flags & (uint32_t)SQZ_FRAME_DICT) != 0 &&
                             (flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_DICT)) == 0) ||
                            (version == 4 && (flags & (uint32_t)SQZ_FRAME_SHUFFLE) != 0 &&
                             (flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_SHUFFLE)) == 0);
    const uint64_t record = version >= 3 ? 8 : 0;           // { dict_bytes, dict_crc } or { elem_bytes, 0 } behind the index
    if (get_le32(frame) != 0x465A5153u || !version_ok || !frame_params_ok(win_bits, block_bits)) { return EINVAL; }
    const uint64_t content = get_le64(frame + 8), payload = get_le64(frame + 16);
    const uint64_t n = get_le32(frame + 24);
    if (frame_blocks(content, block_bits) != n || (payload & 7u) != 0) { return EINVAL; }
    const uint64_t payload_off = frame_payload_off(n, record);      // n < 2^32: no overflow
    if (payload > ~(uint64_t)0 - payload_off) { return EINVAL; }
    out->content_bytes = content;
    out->payload_bytes = payload;
    out->payload_off = payload_off;
    out->frame_bytes = payload_off + payload;
    out->block_bytes = 1ull << block_bits;
    out->n_blocks = (uint32_t)n;
    out->win_bits = win_bits;
    out->version = version;
    out->reserved = flags;
    if (avail >= 32 + 8 * n + record) {                     // the index (and the record) is there: check it too
        const uint32_t crc = host_crc32(host_crc32(0, frame, 28), frame + 32, 8 * n + record);
        if (crc != get_le32(frame + 28)) { return EILSEQ; }
        if (version == 3) {                                 // a dictionary of 1 .. window - 1 bytes
            const uint32_t db = get_le32(frame + 32 + 8 * n);
            if (db == 0 || db > (1u << win_bits) - 1u) { return EINVAL; }
        }
        if (version == 4) {                                 // elements of 2, 4 or 8 bytes, and a zero word
            const uint32_t eb = get_le32(frame + 32 + 8 * n);
            if ((eb != 2 && eb != 4 && eb != 8) || get_le32(frame + 32 + 8 * n + 4) != 0) { return EINVAL; }
        }
        uint64_t words = 0;
        for (uint64_t b = 0; b < n; b++) {                  // < 2^64: n, words < 2^32
            const uint32_t w = frame_entry_words(frame, version, b);
            if (frame_entry_stored(frame, version, b) &&
                ((flags & (uint32_t)SQZ_FRAME_STORED) == 0 ||
                 w != (frame_block_len(content, block_bits, b) + 7) / 8)) { return EINVAL; }
            words += w;
        }
        if (words != payload / 8) { return EINVAL; }
    }
    return 0;
}

int sqz_frame_blocks(const uint8_t* frame, uint64_t avail, uint32_t first, uint32_t count,
                     struct sqz_frame_block* out) {
    struct sqz_frame_info fi;
    const int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    if ((uint64_t)first + count > fi.n_blocks || (out == NULL && count > 0)) { return EINVAL; }
    const uint32_t block_bits = frame[6];
    uint64_t at = fi.payload_off;
    for (uint64_t b = 0; b < (uint64_t)first + count; b++) {
        const uint64_t share = 8 * (uint64_t)frame_entry_words(frame, fi.version, b);
        if (b >= first) {
            struct sqz_frame_block& o = out[b - first];
            o.payload_off = at;
            o.payload_bytes = share;
            o.content_bytes = frame_block_len(fi.content_bytes, block_bits, b);
            o.content_crc = get_le32(frame + 32 + 8 * b + 4);
            o.stored = frame_entry_stored(frame, fi.version, b) ? 1u : 0u;
        }
        at += share;
    }
    return 0;
}

uint64_t sqz_frame_bound_ex(uint64_t content_bytes, uint32_t block_bits, uint32_t flags) {
    if (!frame_flags_ok(flags)) { return 0; }
    if (flags == 0) { return sqz_frame_bound(content_bytes, block_bits); }
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits) { return 0; }
    // no block takes more than its content rounded up to 8 bytes, and all but the last are multiples of 8
    return frame_payload_off(frame_blocks(content_bytes, block_bits)) + align_up(content_bytes, 8);
}

uint64_t sqz_frame_bound_dict(uint64_t content_bytes, uint32_t block_bits, uint32_t flags) {
    if ((flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_DICT)) != 0) { return 0; }
    const uint64_t plain = sqz_frame_bound_ex(content_bytes, block_bits, flags & (uint32_t)SQZ_FRAME_STORED);
    if (plain == 0) { return 0; }
    const uint64_t n = frame_blocks(content_bytes, block_bits);      // the record: 8 bytes more in front of the padding
    return plain - frame_payload_off(n) + frame_payload_off(n, 8);
}

int sqz_frame_dict(const uint8_t* frame, uint64_t avail, uint32_t* dict_bytes, uint32_t* dict_crc) {
    struct sqz_frame_info fi;
    const int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    if (fi.version != 3) { return EINVAL; }
    const uint8_t* const rec = frame + 32 + 8 * (uint64_t)fi.n_blocks;
    if (dict_bytes != NULL) { *dict_bytes = get_le32(rec); }
    if (dict_crc != NULL) { *dict_crc = get_le32(rec + 4); }
    return 0;
}

uint64_t sqz_frame_bound_shuf(uint64_t content_bytes, uint32_t block_bits, uint32_t flags) {
    if ((flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_SHUFFLE)) != 0) { return 0; }
    const uint64_t plain = sqz_frame_bound_ex(content_bytes, block_bits, flags & (uint32_t)SQZ_FRAME_STORED);
    if (plain == 0) { return 0; }
    const uint64_t n = frame_blocks(content_bytes, block_bits);      // the record: 8 bytes more in front of the padding
    return plain - frame_payload_off(n) + frame_payload_off(n, 8);
}

int sqz_frame_elem(const uint8_t* frame, uint64_t avail, uint32_t* elem_bytes) {
    struct sqz_frame_info fi;
    const int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    if (fi.version != 4) { return EINVAL; }
    if (elem_bytes != NULL) { *elem_bytes = get_le32(frame + 32 + 8 * (uint64_t)fi.n_blocks); }
    return 0;
}

int sqz_frame_compress(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                       uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes) {
    return sqz_frame_compress_ex(data, bytes, win_bits, block_bits, 0, frame, capacity, frame_bytes);
}

int sqz_frame_compress_ex(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits, uint32_t flags,
                          uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes) {
    return sqz_frame_compress_parse(data, bytes, win_bits, block_bits, flags, SQZ_PARSE_GREEDY, frame, capacity,
                                    frame_bytes);
}

static int frame_compress_host(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                               uint32_t flags, uint32_t parse, const uint8_t* dict, uint32_t dict_bytes,
                               uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes, uint32_t elem = 0);

int sqz_frame_compress_parse(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                             uint32_t flags, uint32_t parse, uint8_t* frame, uint64_t capacity,
                             uint64_t* frame_bytes) {
    return frame_compress_host(data, bytes, win_bits, block_bits, flags, parse, NULL, 0, frame, capacity, frame_bytes);
}

int sqz_frame_compress_dict(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                            uint32_t flags, uint32_t parse, const uint8_t* dict, uint64_t dict_bytes,
                            uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes) {
    if ((flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_DICT)) != 0 || !frame_params_ok(win_bits, block_bits) ||
        !dict_ok(dict, dict_bytes, 1u << win_bits)) { return EINVAL; }
    return frame_compress_host(data, bytes, win_bits, block_bits, flags & (uint32_t)SQZ_FRAME_STORED, parse, dict,
                               (uint32_t)dict_bytes, frame, capacity, frame_bytes);
}

static bool elem_ok(uint32_t elem_bytes) { return elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8; }
static bool frame_shuf_flags_ok(uint32_t flags) { return (flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_SHUFFLE)) == 0; }

int sqz_frame_compress_shuf(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                            uint32_t flags, uint32_t parse, uint32_t elem_bytes, uint8_t* frame, uint64_t capacity,
                            uint64_t* frame_bytes) {
    if (!frame_shuf_flags_ok(flags) || !frame_params_ok(win_bits, block_bits) || !elem_ok(elem_bytes)) { return EINVAL; }
    return frame_compress_host(data, bytes, win_bits, block_bits, flags & (uint32_t)SQZ_FRAME_STORED, parse, NULL, 0,
                               frame, capacity, frame_bytes, elem_bytes);
}

// dict == NULL and elem == 0: versions 1 and 2 as they always were; a dictionary: version 3, flags | SQZ_FRAME_DICT;
// elem 2, 4 or 8 (and no dictionary): version 4, flags | SQZ_FRAME_SHUFFLE
static int frame_compress_host(const uint8_t* data, uint64_t bytes, uint32_t win_bits, uint32_t block_bits,
                               uint32_t flags, uint32_t parse, const uint8_t* dict, uint32_t dict_bytes,
                               uint8_t* frame, uint64_t capacity, uint64_t* frame_bytes, uint32_t elem) {
    if (!parse_ok(parse)) { return EINVAL; }
    if (frame_bytes == NULL || (frame == NULL && capacity > 0) || (data == NULL && bytes > 0) ||
        !frame_params_ok(win_bits, block_bits) || !frame_flags_ok(flags)) { return EINVAL; }
    const bool store = (flags & SQZ_FRAME_STORED) != 0;
    const uint64_t bb = 1ull << block_bits, n = frame_blocks(bytes, block_bits);
    if (n > 0xFFFFFFFFull) { return EINVAL; }
    const uint64_t record = dict != NULL || elem != 0 ? 8 : 0;
    const uint64_t payload_off = frame_payload_off(n, record), slab = sqz_bound(bb);
    bool fits = capacity >= payload_off;
    std::vector<uint8_t> head(payload_off, 0);              // header, index, padding: built here, copied at the end
    uint64_t payload = 0;
    if (n > 0) {
        int e = device_ready();
        if (e != 0) { return e; }
        LaneLease lease;
        Lane& c = *lease.lane;
        hipStream_t st = lease.stream(nullptr);
        const uint64_t pass = frame_pass_blocks(bb);
        std::vector<uint64_t> out_bytes, dense_off;
        std::vector<int32_t> err;
        std::vector<uint32_t> crc;
        DictDev dd;                                         // uploaded and indexed once, whatever the number of passes
        if (dict != NULL && (e = upload_dict(c, st, dict, dict_bytes, true, &dd)) != 0) { return e; }
        for (uint64_t p0 = 0; p0 < n; p0 += pass) {
            const uint32_t pn = (uint32_t)(n - p0 < pass ? n - p0 : pass);
            const uint64_t c0 = p0 * bb, c1 = (p0 + pn) * bb < bytes ? (p0 + pn) * bb : bytes, total_in = c1 - c0;
            if ((e = c.in.reserve(total_in + 16)) || (e = c.out.reserve((uint64_t)pn * slab + 16)) ||
                (e = c.in_off.reserve(((uint64_t)pn + 1) * 8)) || (e = c.out_off.reserve(((uint64_t)pn + 1) * 8)) ||
                (e = c.tok_count.reserve((size_t)pn * 4)) || (e = c.crc.reserve((size_t)pn * 4)) ||
                (e = c.work_a.reserve((total_in + 64) * 4)) || (e = c.work_m.reserve((total_in + 64) * 4)) ||
                (e = c.out_bytes.reserve((size_t)pn * 8)) || (e = c.err.reserve((size_t)pn * 4))) { return e; }
            HIP_TRY(hipMemcpyAsync(c.in.p, data + c0, total_in, hipMemcpyHostToDevice, st));
            sqzk::launch_frame_plan(pn, bb, total_in, slab, (uint64_t*)c.in_off.p, (uint64_t*)c.out_off.p, st);
            { SpanGuard g(st, SQZ_HIP_K_CRC32);
              sqzk::launch_crc32_blocks((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, pn, (uint32_t*)c.crc.p, bb, st); }
            const uint8_t* enc_in = (const uint8_t*)c.in.p; // version 4: the encoder reads the pass shuffled, total_in + 16
            if (elem != 0) {                                // bytes more on the device; checksums and stored blocks do not
                if ((e = c.shuf.reserve(total_in + 16)) != 0) { return e; }
                sqzk::launch_shuffle_blocks((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, pn, elem, false,
                                            (uint8_t*)c.shuf.p, nullptr, bb, st);
                enc_in = (const uint8_t*)c.shuf.p;
            }
            run_encode(dict != NULL ? 1 : finder_for(parse), enc_in, (const uint64_t*)c.in_off.p, pn,
                       1u << win_bits,
                       (uint32_t*)c.work_a.p, (uint32_t*)c.tok_count.p, (uint32_t*)c.work_a.p, (uint32_t*)c.work_m.p, bb,
                       (uint8_t*)c.out.p, (const uint64_t*)c.out_off.p, (uint64_t*)c.out_bytes.p, (int32_t*)c.err.p,
                       0, 0, total_in + 64, nullptr, st, parse, dict != NULL ? &dd : nullptr);
            HIP_TRY(hipGetLastError());
            out_bytes.resize(pn); err.resize(pn); crc.resize(pn); dense_off.resize((size_t)pn + 1);
            HIP_TRY(hipMemcpyAsync(out_bytes.data(), c.out_bytes.p, (size_t)pn * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(err.data(), c.err.p, (size_t)pn * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(crc.data(), c.crc.p, (size_t)pn * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            dense_off[0] = 0;
            bool any_stored = false;
            for (uint32_t b = 0; b < pn; b++) {
                if (err[b] != 0) { return err[b]; }
                if ((out_bytes[b] & 7u) != 0 || out_bytes[b] / 8 > (store || elem != 0 ? 0x7FFFFFFFull : 0xFFFFFFFFull)) { return EINVAL; }
                const uint64_t len = frame_block_len(bytes, block_bits, p0 + b);
                const bool st_b = store && out_bytes[b] >= len;     // the writer's rule (include/sqz/sqz.h)
                const uint64_t share = st_b ? align_up(len, 8) : out_bytes[b];
                dense_off[b + 1] = dense_off[b] + share;
                put_le32(head.data() + 32 + 8 * (p0 + b), (uint32_t)(share / 8) | (st_b ? 0x80000000u : 0u));
                put_le32(head.data() + 32 + 8 * (p0 + b) + 4, crc[b]);
                crc[b] = st_b ? 1u : 0u;                            // (the checksum is in the index): the copy's mask
                if (st_b) { out_bytes[b] = 0; any_stored = true; }  // from here on: what the compaction moves
            }
            const uint64_t dense_total = dense_off[pn];
            fits = fits && dense_total <= capacity - payload_off - payload;
            if (fits && dense_total > 0) {                  // the pass's streams leave as one transfer to their place
                if ((e = c.dense.reserve(dense_total + 16)) || (e = c.dense_off.reserve(((size_t)pn + 1) * 8))) { return e; }
                HIP_TRY(hipMemcpyAsync(c.dense_off.p, dense_off.data(), ((size_t)pn + 1) * 8, hipMemcpyHostToDevice, st));
                if (any_stored) {                           // the stored blocks: no stream to move, their content instead
                    HIP_TRY(hipMemcpyAsync(c.out_bytes.p, out_bytes.data(), (size_t)pn * 8, hipMemcpyHostToDevice, st));
                    HIP_TRY(hipMemcpyAsync(c.crc.p, crc.data(), (size_t)pn * 4, hipMemcpyHostToDevice, st));
                    SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
                    sqzk::launch_range_copy((const uint8_t*)c.in.p, (const uint64_t*)c.in_off.p, (uint8_t*)c.dense.p,
                                            (const uint64_t*)c.dense_off.p, (const uint64_t*)c.in_off.p,
                                            (const uint32_t*)c.crc.p, pn, true, bb, st);
                }
                sqzk::launch_compact_blocks((const uint8_t*)c.out.p, (const uint64_t*)c.out_off.p,
                                            (const uint64_t*)c.out_bytes.p, pn, (uint8_t*)c.dense.p,
                                            (const uint64_t*)c.dense_off.p, dense_total / pn, st);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(frame + payload_off + payload, c.dense.p, dense_total, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            payload += dense_total;
        }
    }
    *frame_bytes = payload_off + payload;
    if (!fits) { return E2BIG; }
    uint8_t* h = head.data();
    put_le32(h, 0x465A5153u);
    h[4] = elem != 0 ? 4 : dict != NULL ? 3 : store ? 2 : 1; h[5] = (uint8_t)win_bits; h[6] = (uint8_t)block_bits;
    h[7] = (uint8_t)(flags | (dict != NULL ? (uint32_t)SQZ_FRAME_DICT : 0u) | (elem != 0 ? (uint32_t)SQZ_FRAME_SHUFFLE : 0u));
    put_le64(h + 8, bytes);
    put_le64(h + 16, payload);
    put_le32(h + 24, (uint32_t)n);
    if (dict != NULL) {                                     // the record: which dictionary a reader has to bring
        put_le32(h + 32 + 8 * n, dict_bytes);
        put_le32(h + 32 + 8 * n + 4, host_crc32(0, dict, dict_bytes));
    }
    if (elem != 0) { put_le32(h + 32 + 8 * n, elem); }      // the record: { elem_bytes, 0 }
    put_le32(h + 28, host_crc32(host_crc32(0, h, 28), h + 32, 8 * n + record));
    memcpy(frame, h, payload_off);
    return 0;
}

// most_version: 2 for the calls there always were, 4 for the _shuf readers, which take versions 1, 2 and 4
static int frame_decompress_host(const uint8_t* frame, uint64_t avail, uint8_t* data, uint64_t capacity,
                                 uint64_t* bytes, int32_t* block_err, uint32_t most_version);
static int frame_read_host(const uint8_t* frame, uint64_t avail, uint64_t offset, uint64_t length, uint8_t* out,
                           uint32_t most_version);

int sqz_frame_decompress(const uint8_t* frame, uint64_t avail, uint8_t* data, uint64_t capacity,
                         uint64_t* bytes, int32_t* block_err) {
    return frame_decompress_host(frame, avail, data, capacity, bytes, block_err, 2);
}
int sqz_frame_decompress_shuf(const uint8_t* frame, uint64_t avail, uint8_t* data, uint64_t capacity,
                              uint64_t* bytes, int32_t* block_err) {
    return frame_decompress_host(frame, avail, data, capacity, bytes, block_err, 4);
}
int sqz_frame_read(const uint8_t* frame, uint64_t avail, uint64_t offset, uint64_t length, uint8_t* out) {
    return frame_read_host(frame, avail, offset, length, out, 2);
}
int sqz_frame_read_shuf(const uint8_t* frame, uint64_t avail, uint64_t offset, uint64_t length, uint8_t* out) {
    return frame_read_host(frame, avail, offset, length, out, 4);
}

static int frame_decompress_host(const uint8_t* frame, uint64_t avail, uint8_t* data, uint64_t capacity,
                                 uint64_t* bytes, int32_t* block_err, uint32_t most_version) {
    struct sqz_frame_info fi;
    int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    // version 3 needs its dictionary: sqz_frame_decompress_dict; version 4 its inverse shuffle: sqz_frame_decompress_shuf
    if (fi.version == 3 || fi.version > most_version) { return EINVAL; }
    if (bytes != NULL) { *bytes = fi.content_bytes; }
    if (avail < fi.frame_bytes || capacity < fi.content_bytes) { return E2BIG; }
    if (fi.n_blocks == 0) { return 0; }
    if (data == NULL) { return EINVAL; }
    if ((e = device_ready()) != 0) { return e; }
    LaneLease lease;
    hipStream_t st = lease.stream(nullptr);
    int first_bad = 0;
    e = frame_decode_host(*lease.lane, st, frame, fi, 0, fi.n_blocks,
        [&](uint64_t p0, uint64_t pn, const int32_t* errs, const uint8_t* d_bytes, uint64_t count) -> int {
            for (uint64_t k = 0; k < pn; k++) {
                if (block_err != NULL) { block_err[p0 + k] = errs[k]; }
                if (first_bad == 0) { first_bad = errs[k]; }
            }
            if (count > 0) {
                HIP_TRY(hipMemcpyAsync(data + p0 * fi.block_bytes, d_bytes, count, hipMemcpyDeviceToHost, st));
            }
            return 0;
        });
    return e != 0 ? e : first_bad;
}

static int frame_read_host(const uint8_t* frame, uint64_t avail, uint64_t offset, uint64_t length, uint8_t* out,
                           uint32_t most_version) {
    struct sqz_frame_info fi;
    int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    if (fi.version == 3 || fi.version > most_version) { return EINVAL; }   // sqz_frame_read_dict, sqz_frame_read_shuf
    if (offset > fi.content_bytes || length > fi.content_bytes - offset || (out == NULL && length > 0)) { return EINVAL; }
    if (length == 0) { return 0; }
    const uint64_t bb = fi.block_bytes, b_first = offset / bb, b_end = (offset + length - 1) / bb + 1;
    uint64_t words = 0;                                     // the covering streams must be inside avail
    for (uint64_t b = 0; b < b_end; b++) { words += frame_entry_words(frame, fi.version, b); }
    if (8 * words > avail - fi.payload_off) { return E2BIG; }
    if ((e = device_ready()) != 0) { return e; }
    LaneLease lease;
    hipStream_t st = lease.stream(nullptr);
    return frame_decode_host(*lease.lane, st, frame, fi, b_first, b_end,
        [&](uint64_t p0, uint64_t pn, const int32_t* errs, const uint8_t* d_bytes, uint64_t count) -> int {
            for (uint64_t k = 0; k < pn; k++) { if (errs[k] != 0) { return errs[k]; } }
            const uint64_t lo = offset > p0 * bb ? offset : p0 * bb;
            const uint64_t hi = offset + length < p0 * bb + count ? offset + length : p0 * bb + count;
            if (hi > lo) {
                HIP_TRY(hipMemcpyAsync(out + (lo - offset), d_bytes + (lo - p0 * bb), hi - lo, hipMemcpyDeviceToHost, st));
            }
            return 0;
        });
}

// a version-3 frame and the dictionary a reader brought: EINVAL a frame of another version or an impossible
// dictionary, EILSEQ one that is not the writer's (length or checksum)
static int frame_dict_check(const uint8_t* frame, const struct sqz_frame_info& fi, const uint8_t* dict, uint64_t dict_bytes) {
    if (fi.version != 3 || !dict_ok(dict, dict_bytes, 1u << fi.win_bits)) { return EINVAL; }
    const uint8_t* const rec = frame + 32 + 8 * (uint64_t)fi.n_blocks;
    if (get_le32(rec) != dict_bytes || get_le32(rec + 4) != host_crc32(0, dict, dict_bytes)) { return EILSEQ; }
    return 0;
}

int sqz_frame_decompress_dict(const uint8_t* frame, uint64_t avail, const uint8_t* dict, uint64_t dict_bytes,
                              uint8_t* data, uint64_t capacity, uint64_t* bytes, int32_t* block_err) {
    struct sqz_frame_info fi;
    int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    if ((e = frame_dict_check(frame, fi, dict, dict_bytes)) != 0) {
        if (e == EILSEQ && block_err != NULL) { for (uint32_t b = 0; b < fi.n_blocks; b++) { block_err[b] = EILSEQ; } }
        return e;
    }
    if (bytes != NULL) { *bytes = fi.content_bytes; }
    if (avail < fi.frame_bytes || capacity < fi.content_bytes) { return E2BIG; }
    if (fi.n_blocks == 0) { return 0; }
    if (data == NULL) { return EINVAL; }
    if ((e = device_ready()) != 0) { return e; }
    LaneLease lease;
    hipStream_t st = lease.stream(nullptr);
    DictDev dd;
    if ((e = upload_dict(*lease.lane, st, dict, (uint32_t)dict_bytes, false, &dd)) != 0) { return e; }
    int first_bad = 0;
    e = frame_decode_host_dict(*lease.lane, st, frame, fi, 0, fi.n_blocks, dd,
        [&](uint64_t p0, uint64_t pn, const int32_t* errs, const uint8_t* d_bytes, uint64_t count) -> int {
            for (uint64_t k = 0; k < pn; k++) {
                if (block_err != NULL) { block_err[p0 + k] = errs[k]; }
                if (first_bad == 0) { first_bad = errs[k]; }
            }
            if (count > 0) {
                HIP_TRY(hipMemcpyAsync(data + p0 * fi.block_bytes, d_bytes, count, hipMemcpyDeviceToHost, st));
            }
            return 0;
        });
    return e != 0 ? e : first_bad;
}

int sqz_frame_read_dict(const uint8_t* frame, uint64_t avail, const uint8_t* dict, uint64_t dict_bytes,
                        uint64_t offset, uint64_t length, uint8_t* out) {
    struct sqz_frame_info fi;
    int e = frame_check_host(frame, avail, &fi);
    if (e != 0) { return e; }
    if ((e = frame_dict_check(frame, fi, dict, dict_bytes)) != 0) { return e; }
    if (offset > fi.content_bytes || length > fi.content_bytes - offset || (out == NULL && length > 0)) { return EINVAL; }
    if (length == 0) { return 0; }
    const uint64_t bb = fi.block_bytes, b_first = offset / bb, b_end = (offset + length - 1) / bb + 1;
    uint64_t words = 0;                                     // the covering streams must be inside avail
    for (uint64_t b = 0; b < b_end; b++) { words += frame_entry_words(frame, fi.version, b); }
    if (8 * words > avail - fi.payload_off) { return E2BIG; }
    if ((e = device_ready()) != 0) { return e; }
    LaneLease lease;
    hipStream_t st = lease.stream(nullptr);
    DictDev dd;
    if ((e = upload_dict(*lease.lane, st, dict, (uint32_t)dict_bytes, false, &dd)) != 0) { return e; }
    return frame_decode_host_dict(*lease.lane, st, frame, fi, b_first, b_end, dd,
        [&](uint64_t p0, uint64_t pn, const int32_t* errs, const uint8_t* d_bytes, uint64_t count) -> int {
            for (uint64_t k = 0; k < pn; k++) { if (errs[k] != 0) { return errs[k]; } }
            const uint64_t lo = offset > p0 * bb ? offset : p0 * bb;
            const uint64_t hi = offset + length < p0 * bb + count ? offset + length : p0 * bb + count;
            if (hi > lo) {
                HIP_TRY(hipMemcpyAsync(out + (lo - offset), d_bytes + (lo - p0 * bb), hi - lo, hipMemcpyDeviceToHost, st));
            }
            return 0;
        });
}

uint64_t sqz_hip_frame_scratch_bytes(uint64_t content_bytes, uint32_t block_bits, int encode) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits) { return 0; }
    const uint64_t n = frame_blocks(content_bytes, block_bits);
    return frame_scratch(n, content_bytes, sqz_bound(1ull << block_bits), encode != 0).total;
}

uint64_t sqz_hip_frame_scratch_bytes_ex(uint64_t content_bytes, uint32_t block_bits, int encode, uint32_t flags) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        !frame_flags_ok(flags)) { return 0; }
    const uint64_t n = frame_blocks(content_bytes, block_bits);
    return frame_scratch(n, content_bytes, sqz_bound(1ull << block_bits), encode != 0,
                         (flags & SQZ_FRAME_STORED) != 0).total;
}

int sqz_hip_frame_encode(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                         void* d_frame, uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status,
                         int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return sqz_hip_frame_encode_ex(d_in, content_bytes, win_bits, block_bits, 0, d_frame, capacity, d_frame_bytes,
                                   d_status, d_err, d_scratch, scratch_bytes, stream);
}

int sqz_hip_frame_encode_ex(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                            uint32_t flags, void* d_frame, uint64_t capacity, uint64_t* d_frame_bytes,
                            int32_t* d_status, int32_t* d_err, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return sqz_hip_frame_encode_parse(d_in, content_bytes, win_bits, block_bits, flags, SQZ_PARSE_GREEDY, d_frame,
                                      capacity, d_frame_bytes, d_status, d_err, d_scratch, scratch_bytes, stream);
}

int sqz_hip_frame_encode_parse(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                               uint32_t flags, uint32_t parse, void* d_frame, uint64_t capacity,
                               uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err, void* d_scratch,
                               uint64_t scratch_bytes, void* stream) {
    if (!parse_ok(parse)) { return EINVAL; }
    if (!frame_flags_ok(flags)) { return EINVAL; }
    if (!frame_params_ok(win_bits, block_bits) || (d_in == NULL && content_bytes > 0) || d_frame == NULL ||
        ((uintptr_t)d_frame & 15u) != 0 || d_frame_bytes == NULL || d_status == NULL ||
        (d_err == NULL && content_bytes > 0) || d_scratch == NULL || ((uintptr_t)d_scratch & 15u) != 0) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    return frame_encode_dev((const uint8_t*)d_in, content_bytes, win_bits, block_bits, (uint8_t*)d_frame, capacity,
                            d_frame_bytes, d_status, d_err, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                            flags, parse);
}

int sqz_hip_frame_decode(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                         void* d_out, int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                         void* stream) {
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_status == NULL || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0 || (n_blocks > 0 && (d_out == NULL || d_err == NULL)) ||
        (n_blocks == 0) != (content_bytes == 0) || content_bytes / (1ull << sqz_frame_min_block_bits) + 1 < n_blocks) {
        return EINVAL;
    }
    if (avail < 32 + 8 * (uint64_t)n_blocks) { return E2BIG; }
    const int e = device_ready();
    if (e != 0) { return e; }
    return frame_decode_dev((const uint8_t*)d_frame, avail, n_blocks, content_bytes, 0, n_blocks, content_bytes,
                            (uint8_t*)d_out, d_err, d_status, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                            0);
}

// ---- version 3 in the device-resident flavour, and ranged reads from a resident frame
static bool frame_dict_flags_ok(uint32_t flags) { return (flags & ~(uint32_t)(SQZ_FRAME_STORED | SQZ_FRAME_DICT)) == 0; }

uint64_t sqz_hip_frame_scratch_bytes_dict(uint64_t content_bytes, uint32_t block_bits, int encode, uint32_t flags,
                                          uint64_t dict_bytes) {
    if (!frame_dict_flags_ok(flags) || dict_bytes < 1 || dict_bytes > (uint64_t)sqzk_max_window - 1) { return 0; }
    const uint64_t plain = sqz_hip_frame_scratch_bytes_ex(content_bytes, block_bits, encode,
                                                          encode != 0 ? flags & (uint32_t)SQZ_FRAME_STORED : 0u);
    if (plain == 0) { return 0; }
    return encode != 0 ? plain + dict_index_bytes(dict_bytes) : plain;
}

int sqz_hip_frame_encode_dict(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                              uint32_t flags, uint32_t parse, const void* d_dict, uint64_t dict_bytes, void* d_frame,
                              uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err,
                              void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!parse_ok(parse) || !frame_dict_flags_ok(flags) || !frame_params_ok(win_bits, block_bits) ||
        !dict_ok(d_dict, dict_bytes, 1u << win_bits)) { return EINVAL; }
    if ((d_in == NULL && content_bytes > 0) || d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 ||
        d_frame_bytes == NULL || d_status == NULL || (d_err == NULL && content_bytes > 0) || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    return frame_encode_dev((const uint8_t*)d_in, content_bytes, win_bits, block_bits, (uint8_t*)d_frame, capacity,
                            d_frame_bytes, d_status, d_err, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                            flags & (uint32_t)SQZ_FRAME_STORED, parse, (const uint8_t*)d_dict, (uint32_t)dict_bytes);
}

int sqz_hip_frame_decode_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                              const void* d_dict, uint64_t dict_bytes, void* d_out, int32_t* d_err, int32_t* d_status,
                              void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!dict_ok(d_dict, dict_bytes, (uint32_t)sqzk_max_window)) { return EINVAL; }
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_status == NULL || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0 || (n_blocks > 0 && (d_out == NULL || d_err == NULL)) ||
        (n_blocks == 0) != (content_bytes == 0) || content_bytes / (1ull << sqz_frame_min_block_bits) + 1 < n_blocks) {
        return EINVAL;
    }
    if (avail < 32 + 8 * (uint64_t)n_blocks + 8) { return E2BIG; }
    const int e = device_ready();
    if (e != 0) { return e; }
    return frame_decode_dev((const uint8_t*)d_frame, avail, n_blocks, content_bytes, 0, n_blocks, content_bytes,
                            (uint8_t*)d_out, d_err, d_status, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                            0, (const uint8_t*)d_dict, (uint32_t)dict_bytes);
}

uint64_t sqz_hip_frame_read_scratch_bytes(uint64_t length, uint32_t block_bits) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits) { return 0; }
    const uint64_t bb = 1ull << block_bits;
    if (length > ~(uint64_t)0 / 8 - 2 * bb) { return 0; }
    // a range that starts at a block's last byte covers the most blocks
    const uint64_t n = length == 0 ? 0 : ((length + bb - 2) >> block_bits) + 1;
    return read_scratch(n, n * bb).total;
}

// dict == NULL: versions 1 and 2 (sqz_hip_frame_read); else version 3
static int frame_read_call(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                           uint32_t block_bits, uint64_t offset, uint64_t length, const void* d_dict,
                           uint64_t dict_bytes, void* d_out, int32_t* d_err, int32_t* d_status, void* d_scratch,
                           uint64_t scratch_bytes, void* stream, uint32_t elem = 0) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        frame_blocks(content_bytes, block_bits) != n_blocks || offset > content_bytes ||
        length > content_bytes - offset) { return EINVAL; }
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_status == NULL || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0 || (length > 0 && (d_out == NULL || d_err == NULL))) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    if (length == 0) { return hip_errno(hipMemsetAsync(d_status, 0, 4, (hipStream_t)stream)); }
    return frame_read_dev((const uint8_t*)d_frame, avail, n_blocks, content_bytes, block_bits, offset, length,
                          (uint8_t*)d_out, d_err, d_status, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                          (const uint8_t*)d_dict, (uint32_t)dict_bytes, elem);
}

int sqz_hip_frame_read(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                       uint32_t block_bits, uint64_t offset, uint64_t length, void* d_out, int32_t* d_err,
                       int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return frame_read_call(d_frame, avail, n_blocks, content_bytes, block_bits, offset, length, NULL, 0, d_out, d_err,
                           d_status, d_scratch, scratch_bytes, stream);
}

int sqz_hip_frame_read_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                            uint32_t block_bits, uint64_t offset, uint64_t length, const void* d_dict,
                            uint64_t dict_bytes, void* d_out, int32_t* d_err, int32_t* d_status, void* d_scratch,
                            uint64_t scratch_bytes, void* stream) {
    if (!dict_ok(d_dict, dict_bytes, (uint32_t)sqzk_max_window)) { return EINVAL; }
    return frame_read_call(d_frame, avail, n_blocks, content_bytes, block_bits, offset, length, d_dict, dict_bytes,
                           d_out, d_err, d_status, d_scratch, scratch_bytes, stream);
}

// ---- version 4 in the device-resident flavour
// encode: sqz_hip_frame_scratch_bytes_ex(c, b, 1, flags & SQZ_FRAME_STORED) + round_up_256(c + 16), the shuffled content;
// decode: sqz_hip_frame_scratch_bytes(c, b, 0) + round_up_256(c + 16), the blocks as the decoder leaves them
uint64_t sqz_hip_frame_scratch_bytes_shuf(uint64_t content_bytes, uint32_t block_bits, int encode, uint32_t flags) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        !frame_shuf_flags_ok(flags) || content_bytes > ~(uint64_t)0 / 16) { return 0; }
    const uint64_t n = frame_blocks(content_bytes, block_bits);
    return frame_scratch(n, content_bytes, sqz_bound(1ull << block_bits), encode != 0,
                         encode != 0 && (flags & SQZ_FRAME_STORED) != 0, true).total;
}

int sqz_hip_frame_encode_shuf(const void* d_in, uint64_t content_bytes, uint32_t win_bits, uint32_t block_bits,
                              uint32_t flags, uint32_t parse, uint32_t elem_bytes, void* d_frame, uint64_t capacity,
                              uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err, void* d_scratch,
                              uint64_t scratch_bytes, void* stream) {
    if (!parse_ok(parse) || !frame_shuf_flags_ok(flags) || !frame_params_ok(win_bits, block_bits) ||
        !elem_ok(elem_bytes)) { return EINVAL; }
    if ((d_in == NULL && content_bytes > 0) || d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 ||
        d_frame_bytes == NULL || d_status == NULL || (d_err == NULL && content_bytes > 0) || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0 ||
        scratch_bytes < sqz_hip_frame_scratch_bytes_shuf(content_bytes, block_bits, 1, flags)) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    return frame_encode_dev((const uint8_t*)d_in, content_bytes, win_bits, block_bits, (uint8_t*)d_frame, capacity,
                            d_frame_bytes, d_status, d_err, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                            flags & (uint32_t)SQZ_FRAME_STORED, parse, nullptr, 0, elem_bytes);
}

int sqz_hip_frame_decode_shuf(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                              uint32_t elem_bytes, void* d_out, int32_t* d_err, int32_t* d_status, void* d_scratch,
                              uint64_t scratch_bytes, void* stream) {
    if (!elem_ok(elem_bytes)) { return EINVAL; }
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_status == NULL || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0 || (n_blocks > 0 && (d_out == NULL || d_err == NULL)) ||
        (n_blocks == 0) != (content_bytes == 0) || content_bytes / (1ull << sqz_frame_min_block_bits) + 1 < n_blocks) {
        return EINVAL;
    }
    if (scratch_bytes < frame_scratch(n_blocks, content_bytes, 0, false, false, true).total) { return EINVAL; }
    if (avail < 32 + 8 * (uint64_t)n_blocks + 8) { return E2BIG; }
    const int e = device_ready();
    if (e != 0) { return e; }
    return frame_decode_dev((const uint8_t*)d_frame, avail, n_blocks, content_bytes, 0, n_blocks, content_bytes,
                            (uint8_t*)d_out, d_err, d_status, (uint8_t*)d_scratch, scratch_bytes, (hipStream_t)stream,
                            0, nullptr, 0, 0, elem_bytes);
}

// sqz_hip_frame_read_scratch_bytes(length, b) + round_up_256((k << b) + 16): the covering blocks once more, shuffled
uint64_t sqz_hip_frame_read_scratch_bytes_shuf(uint64_t length, uint32_t block_bits) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits) { return 0; }
    const uint64_t bb = 1ull << block_bits;
    if (length > ~(uint64_t)0 / 16 - 2 * bb) { return 0; }
    const uint64_t n = length == 0 ? 0 : ((length + bb - 2) >> block_bits) + 1;
    return read_scratch(n, n * bb, true).total;
}

int sqz_hip_frame_read_shuf(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                            uint32_t block_bits, uint32_t elem_bytes, uint64_t offset, uint64_t length, void* d_out,
                            int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!elem_ok(elem_bytes)) { return EINVAL; }
    return frame_read_call(d_frame, avail, n_blocks, content_bytes, block_bits, offset, length, NULL, 0, d_out, d_err,
                           d_status, d_scratch, scratch_bytes, stream, elem_bytes);
}

// ---- many ranges of a resident frame in one call
// where the pieces of a gather's scratch lie (every piece 256-byte aligned); m = min(max_blocks, n_blocks) slots
struct GatherScratch {
    uint64_t bitmap, wpre, misc, sel, in_off, out_off, skip, stored, crc, err, src_off, mask, codec, codec_bytes, blocks, total;
};
// with_codec = false leaves the decoder's scratch out (codec = 0, codec_bytes still says what it takes): an update
// places one area for the decoder and the encoder behind its own pieces
static GatherScratch gather_scratch(uint64_t n, uint64_t r, uint64_t m, uint32_t block_bits, bool with_codec = true) {
    GatherScratch G = {};
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) { const uint64_t v = at; at += align_up(bytes, 256); return v; };
    const uint64_t words = (n + 31) / 32;
    G.bitmap = take(words * 4 + 4);
    G.wpre = take(words * 4 + 4);
    G.misc = take(256);                 // as a decode's, and [160,168) count and verdict of the select kernel
    G.sel = take(m * 4 + 4);
    G.in_off = take((2 * m + 1) * 8);   // two entries per slot: the block, and the gap behind its stream
    G.out_off = take((2 * m + 1) * 8);
    G.skip = take(2 * m * 4 + 4);
    G.stored = take(2 * m * 4 + 4);
    G.crc = take(2 * m * 4 + 4);
    G.err = take(2 * m * 4 + 4);
    G.src_off = take(r * 8 + 8);
    G.mask = take(r * 4 + 4);
    G.codec_bytes = sqz_hip_decode_scratch_bytes((uint32_t)(2 * m), m << block_bits);
    G.codec = with_codec ? take(G.codec_bytes) : 0;
    G.blocks = take((m << block_bits) + 16);
    G.total = at;
    return G;
}

uint64_t sqz_hip_frame_gather_scratch_bytes(uint32_t n_blocks, uint32_t n_ranges, uint32_t max_blocks, uint32_t block_bits) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits) { return 0; }
    return gather_scratch(n_blocks, n_ranges, max_blocks < n_blocks ? max_blocks : n_blocks, block_bits).total;
}

// dict == NULL: versions 1 and 2 (sqz_hip_frame_gather); else version 3
static int frame_gather_call(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                             uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length, uint32_t n_ranges,
                             uint64_t max_length, uint32_t max_blocks, const void* d_dict, uint64_t dict_bytes,
                             void* d_out, uint64_t out_capacity, uint64_t* d_out_off, int32_t* d_range_err,
                             uint32_t* d_blocks_decoded, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                             void* stream) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        frame_blocks(content_bytes, block_bits) != n_blocks) { return EINVAL; }
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_scratch == NULL || ((uintptr_t)d_scratch & 15u) != 0 ||
        d_status == NULL || d_blocks_decoded == NULL || d_out_off == NULL ||
        (n_ranges > 0 && (d_offset == NULL || d_length == NULL || d_range_err == NULL)) ||
        (max_blocks > 0 && d_out == NULL)) { return EINVAL; }
    const uint32_t m = max_blocks < n_blocks ? max_blocks : n_blocks;
    const GatherScratch G = gather_scratch(n_blocks, n_ranges, m, block_bits);
    if (scratch_bytes < G.total) { return EINVAL; }
    const uint64_t record = d_dict != NULL ? 8 : 0;
    if (avail < 32 + 8 * (uint64_t)n_blocks + record) { return E2BIG; }
    const int e = device_ready();
    if (e != 0) { return e; }
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* const frame = (const uint8_t*)d_frame;
    uint8_t* const scratch = (uint8_t*)d_scratch;
    uint32_t* bitmap = (uint32_t*)(scratch + G.bitmap);
    uint32_t* wpre = (uint32_t*)(scratch + G.wpre);
    uint64_t* idx_off = (uint64_t*)(scratch + G.misc);
    uint32_t* idx_crc = (uint32_t*)(scratch + G.misc + 16);
    uint64_t* spare = (uint64_t*)(scratch + G.misc + 32);
    uint32_t* ctl = (uint32_t*)(scratch + G.misc + 160);
    uint32_t* sel = (uint32_t*)(scratch + G.sel);
    uint64_t* in_off = (uint64_t*)(scratch + G.in_off);
    uint64_t* out_off = (uint64_t*)(scratch + G.out_off);
    uint32_t* skip = (uint32_t*)(scratch + G.skip);
    uint32_t* stored = (uint32_t*)(scratch + G.stored);
    uint32_t* crc = (uint32_t*)(scratch + G.crc);
    int32_t* err = (int32_t*)(scratch + G.err);
    uint64_t* src_off = (uint64_t*)(scratch + G.src_off);
    uint32_t* mask = (uint32_t*)(scratch + G.mask);
    uint8_t* blocks = scratch + G.blocks;
    // the covering blocks as a bitmap, then as a list, with the output's layout and the verdict on the two caps
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_gather_mark(d_offset, d_length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, st);
      sqzk::launch_gather_select(bitmap, n_blocks, d_offset, d_length, n_ranges, max_length, content_bytes, m,
                                 out_capacity, wpre, sel, d_out_off, ctl, st); }
    // the frame's checks as in frame_decode_dev, and offsets for the list
    const uint64_t idx_bytes = 8 * (uint64_t)n_blocks + record;
    sqzk::launch_frame_plan(1, idx_bytes, idx_bytes, 0, idx_off, spare, st);
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, idx_crc, idx_bytes, st); }
    DictDev dd;
    uint32_t* dict_crc = nullptr;
    if (d_dict != NULL) {
        uint64_t* dict_off = (uint64_t*)(scratch + G.misc + 64);
        dict_crc = (uint32_t*)(scratch + G.misc + 128);
        sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, dict_off, dict_off + 4, st);
        SpanGuard g(st, SQZ_HIP_K_CRC32);
        sqzk::launch_crc32_blocks((const uint8_t*)d_dict, dict_off, 1, dict_crc, dict_bytes, st);
        dd.bytes = (const uint8_t*)d_dict; dd.len = (uint32_t)dict_bytes;
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_frame_open_list(frame, avail, n_blocks, content_bytes, idx_crc, (uint32_t)dict_bytes, dict_crc, bitmap,
                                   wpre, sel, ctl, m, in_off, out_off, skip, stored, d_status, d_blocks_decoded, st,
                                   block_bits); }
    if (m > 0 && n_ranges > 0) {
        uint32_t* counts = (uint32_t*)(scratch + G.codec);
        uint32_t* tokens = (uint32_t*)(scratch + G.codec + align_up((uint64_t)(2 * m) * 4, 256));
        run_frame_decode(frame, in_off, out_off, 2 * m, 1ull << block_bits, tokens, counts, blocks, err, skip, stored, crc,
                         dd, st, m);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_gather_plan(frame, d_offset, d_length, n_ranges, max_length, content_bytes, block_bits, n_blocks,
                               bitmap, wpre, err, crc, d_status, d_range_err, src_off, mask, st); }
    if (m > 0 && n_ranges > 0) {
        SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
        if (max_length <= (uint64_t)sqzk_gather_copy_max) {
            sqzk::launch_gather_copy(blocks, src_off, (uint8_t*)d_out, d_out_off, d_out_off, mask, n_ranges, st);
        } else {
            sqzk::launch_range_copy(blocks, src_off, (uint8_t*)d_out, d_out_off, d_out_off, mask, n_ranges, false,
                                    max_length, st);
        }
    }
    return hip_errno(hipGetLastError());
}

int sqz_hip_frame_gather(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                         uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length, uint32_t n_ranges,
                         uint64_t max_length, uint32_t max_blocks, void* d_out, uint64_t out_capacity,
                         uint64_t* d_out_off, int32_t* d_range_err, uint32_t* d_blocks_decoded, int32_t* d_status,
                         void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return frame_gather_call(d_frame, avail, n_blocks, content_bytes, block_bits, d_offset, d_length, n_ranges,
                             max_length, max_blocks, NULL, 0, d_out, out_capacity, d_out_off, d_range_err,
                             d_blocks_decoded, d_status, d_scratch, scratch_bytes, stream);
}

int sqz_hip_frame_gather_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                              uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length,
                              uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks, const void* d_dict,
                              uint64_t dict_bytes, void* d_out, uint64_t out_capacity, uint64_t* d_out_off,
                              int32_t* d_range_err, uint32_t* d_blocks_decoded, int32_t* d_status, void* d_scratch,
                              uint64_t scratch_bytes, void* stream) {
    if (!dict_ok(d_dict, dict_bytes, (uint32_t)sqzk_max_window)) { return EINVAL; }
    return frame_gather_call(d_frame, avail, n_blocks, content_bytes, block_bits, d_offset, d_length, n_ranges,
                             max_length, max_blocks, d_dict, dict_bytes, d_out, out_capacity, d_out_off, d_range_err,
                             d_blocks_decoded, d_status, d_scratch, scratch_bytes, stream);
}

// ---- many ranges written into a resident frame in one call
// where the pieces of an update's scratch lie (every piece 256-byte aligned): a gather's, a second offset per range,
// and what the encode of the m slots and the merge take.  The encoder's scratch lies over the decoder's.
struct UpdateScratch {
    GatherScratch G;
    uint64_t dst_off, enc_in_off, slab_off, out_bytes, enc_err, crc_new, seg_dst, seg_src, seg_len, verdict, dict_idx,
             slabs, codec, codec_bytes, enc_codec_bytes, total;
};
static UpdateScratch update_scratch(uint64_t n, uint64_t r, uint64_t m, uint32_t block_bits, uint64_t dict_bytes) {
    UpdateScratch U = {};
    // a gather's pieces without its codec area: the larger of the decoder's and the encoder's goes at the end
    U.G = gather_scratch(n, r, m, block_bits, false);
    uint64_t at = U.G.total;
    auto take = [&at](uint64_t bytes) { const uint64_t v = at; at += align_up(bytes, 256); return v; };
    U.dst_off = take(r * 8 + 8);
    U.enc_in_off = take((m + 1) * 8);
    U.slab_off = take((m + 1) * 8);
    U.out_bytes = take(m * 8 + 8);
    U.enc_err = take(m * 4 + 4);
    U.crc_new = take(m * 4 + 4);
    U.seg_dst = take((2 * m + 2) * 8);
    U.seg_src = take((2 * m + 1) * 8);
    U.seg_len = take((2 * m + 1) * 8);
    U.verdict = take(256);
    U.dict_idx = take(dict_bytes != 0 ? dict_index_bytes(dict_bytes) : 0);
    U.slabs = take(m * sqz_bound(1ull << block_bits));
    U.enc_codec_bytes = sqz_hip_encode_scratch_bytes((uint32_t)m, m << block_bits);
    U.codec_bytes = U.G.codec_bytes > U.enc_codec_bytes ? U.G.codec_bytes : U.enc_codec_bytes;
    U.codec = take(U.codec_bytes);
    U.total = at;
    return U;
}

uint64_t sqz_hip_frame_update_scratch_bytes(uint32_t n_blocks, uint32_t n_ranges, uint32_t max_blocks, uint32_t block_bits,
                                            uint64_t dict_bytes) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        dict_bytes > (uint64_t)sqzk_max_window - 1) { return 0; }
    return update_scratch(n_blocks, n_ranges, max_blocks < n_blocks ? max_blocks : n_blocks, block_bits, dict_bytes).total;
}

static bool spans_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a_bytes != 0 && b_bytes != 0 && x < y + b_bytes && y < x + a_bytes;
}

// dict == NULL: versions 1 and 2 (sqz_hip_frame_update); else version 3
static int frame_update_call(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                             uint32_t win_bits, uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length,
                             uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks, const void* d_data,
                             uint64_t data_bytes, uint64_t* d_data_off, uint32_t parse, const void* d_dict,
                             uint64_t dict_bytes, void* d_new_frame, uint64_t capacity, uint64_t* d_frame_bytes,
                             int32_t* d_range_err, uint32_t* d_blocks_encoded, int32_t* d_status, void* d_scratch,
                             uint64_t scratch_bytes, void* stream) {
    if (!frame_params_ok(win_bits, block_bits) || frame_blocks(content_bytes, block_bits) != n_blocks ||
        !parse_ok(parse)) { return EINVAL; }
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_scratch == NULL || ((uintptr_t)d_scratch & 15u) != 0 ||
        d_new_frame == NULL || ((uintptr_t)d_new_frame & 15u) != 0 || d_frame_bytes == NULL ||
        d_status == NULL || d_blocks_encoded == NULL || d_data_off == NULL ||
        (n_ranges > 0 && (d_offset == NULL || d_length == NULL || d_range_err == NULL)) ||
        (data_bytes > 0 && d_data == NULL)) { return EINVAL; }
    const uint32_t m = max_blocks < n_blocks ? max_blocks : n_blocks;
    const UpdateScratch U = update_scratch(n_blocks, n_ranges, m, block_bits, d_dict != NULL ? dict_bytes : 0);
    if (scratch_bytes < U.total) { return EINVAL; }
    if (spans_overlap(d_new_frame, capacity, d_frame, avail) ||
        spans_overlap(d_new_frame, capacity, d_scratch, scratch_bytes)) { return EINVAL; }
    const uint64_t record = d_dict != NULL ? 8 : 0;
    if (avail < 32 + 8 * (uint64_t)n_blocks + record) { return E2BIG; }
    const int e = device_ready();
    if (e != 0) { return e; }
    hipStream_t st = (hipStream_t)stream;
    const GatherScratch& G = U.G;
    const uint8_t* const frame = (const uint8_t*)d_frame;
    uint8_t* const new_frame = (uint8_t*)d_new_frame;
    uint8_t* const scratch = (uint8_t*)d_scratch;
    uint32_t* bitmap = (uint32_t*)(scratch + G.bitmap);
    uint32_t* wpre = (uint32_t*)(scratch + G.wpre);
    uint64_t* idx_off = (uint64_t*)(scratch + G.misc);
    uint32_t* idx_crc = (uint32_t*)(scratch + G.misc + 16);
    uint64_t* spare = (uint64_t*)(scratch + G.misc + 32);
    uint32_t* ctl = (uint32_t*)(scratch + G.misc + 160);      // [160,172): count, verdict, "win_bits is another"
    uint32_t* sel = (uint32_t*)(scratch + G.sel);
    uint64_t* in_off = (uint64_t*)(scratch + G.in_off);
    uint64_t* out_off = (uint64_t*)(scratch + G.out_off);
    uint32_t* skip = (uint32_t*)(scratch + G.skip);
    uint32_t* stored = (uint32_t*)(scratch + G.stored);
    uint32_t* crc = (uint32_t*)(scratch + G.crc);
    int32_t* err = (int32_t*)(scratch + G.err);
    uint64_t* src_off = (uint64_t*)(scratch + G.src_off);
    uint32_t* mask = (uint32_t*)(scratch + G.mask);
    uint8_t* slots = scratch + G.blocks;
    uint64_t* dst_off = (uint64_t*)(scratch + U.dst_off);
    uint64_t* enc_in_off = (uint64_t*)(scratch + U.enc_in_off);
    uint64_t* slab_off = (uint64_t*)(scratch + U.slab_off);
    uint64_t* out_bytes = (uint64_t*)(scratch + U.out_bytes);
    int32_t* enc_err = (int32_t*)(scratch + U.enc_err);
    uint32_t* crc_new = (uint32_t*)(scratch + U.crc_new);
    uint64_t* seg_dst = (uint64_t*)(scratch + U.seg_dst);
    uint64_t* seg_src = (uint64_t*)(scratch + U.seg_src);
    uint64_t* seg_len = (uint64_t*)(scratch + U.seg_len);
    uint32_t* flags = (uint32_t*)(scratch + U.verdict);
    uint64_t* new_idx_off = (uint64_t*)(scratch + U.verdict + 16);
    uint32_t* new_idx_crc = (uint32_t*)(scratch + U.verdict + 32);
    uint8_t* slabs = scratch + U.slabs;
    const uint64_t bb = 1ull << block_bits, slab = sqz_bound(bb);
    // the covering blocks as a bitmap and a list, the data's layout, the patch's work list, the verdict on the request
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_gather_mark(d_offset, d_length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, st);
      sqzk::launch_gather_select(bitmap, n_blocks, d_offset, d_length, n_ranges, max_length, content_bytes, m,
                                 data_bytes, wpre, sel, d_data_off, ctl, st);
      sqzk::launch_update_plan(d_offset, d_length, n_ranges, max_length, content_bytes, block_bits, n_blocks, bitmap, wpre,
                               d_data_off, d_range_err, src_off, dst_off, mask, frame, win_bits, flags, ctl, st); }
    // the frame's checks and the touched blocks into their slots, as a gather's
    const uint64_t idx_bytes = 8 * (uint64_t)n_blocks + record;
    sqzk::launch_frame_plan(1, idx_bytes, idx_bytes, 0, idx_off, spare, st);
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, idx_crc, idx_bytes, st); }
    DictDev dd;
    uint32_t* dict_crc = nullptr;
    if (d_dict != NULL) {
        uint64_t* dict_off = (uint64_t*)(scratch + G.misc + 64);
        dict_crc = (uint32_t*)(scratch + G.misc + 128);
        sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, dict_off, dict_off + 4, st);
        SpanGuard g(st, SQZ_HIP_K_CRC32);
        sqzk::launch_crc32_blocks((const uint8_t*)d_dict, dict_off, 1, dict_crc, dict_bytes, st);
        dd.bytes = (const uint8_t*)d_dict; dd.len = (uint32_t)dict_bytes;
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_frame_open_list(frame, avail, n_blocks, content_bytes, idx_crc, (uint32_t)dict_bytes, dict_crc, bitmap,
                                   wpre, sel, ctl, m, in_off, out_off, skip, stored, d_status, d_blocks_encoded, st,
                                   block_bits); }
    const bool work = m > 0 && n_ranges > 0;
    if (work) {
        uint32_t* counts = (uint32_t*)(scratch + U.codec);
        uint32_t* tokens = (uint32_t*)(scratch + U.codec + align_up((uint64_t)(2 * m) * 4, 256));
        run_frame_decode(frame, in_off, out_off, 2 * m, bb, tokens, counts, slots, err, skip, stored, crc, dd, st, m);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_update_verdict(frame, sel, ctl, m, err, crc, block_bits, content_bytes, slab, n_ranges, d_status,
                                  d_blocks_encoded, mask, enc_in_off, slab_off, st); }
    if (work) {
        { SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);                // the patch: the data into the slots
          if (max_length <= (uint64_t)sqzk_gather_copy_max) {
              sqzk::launch_gather_copy((const uint8_t*)d_data, src_off, slots, dst_off, d_data_off, mask, n_ranges, st);
          } else {
              sqzk::launch_range_copy((const uint8_t*)d_data, src_off, slots, dst_off, d_data_off, mask, n_ranges, false,
                                      max_length, st);
          } }
        { SpanGuard g(st, SQZ_HIP_K_CRC32);
          sqzk::launch_crc32_blocks(slots, enc_in_off, m, crc_new, bb, st); }
        if (d_dict != NULL) { dd = run_dict_index((const uint8_t*)d_dict, (uint32_t)dict_bytes, scratch + U.dict_idx, st); }
        const uint64_t head = align_up((uint64_t)m * 4, 256);
        const uint64_t slots_n = (U.enc_codec_bytes - head) / 8;
        uint32_t* counts = (uint32_t*)(scratch + U.codec);
        uint32_t* tokens = (uint32_t*)(scratch + U.codec + head);
        run_encode(d_dict != NULL ? 1 : finder_for(parse), slots, enc_in_off, m, 1u << win_bits, tokens, counts, tokens,
                   tokens + slots_n, bb, slabs, slab_off, out_bytes, enc_err, 0, 0, slots_n, nullptr, st, parse,
                   d_dict != NULL ? &dd : nullptr);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_frame_merge_index(frame, n_blocks, content_bytes, d_dict != NULL, bitmap, wpre, ctl, m, out_bytes, enc_err,
                                     crc_new, slab, new_frame, capacity, seg_dst, seg_src, seg_len, new_idx_off,
                                     d_frame_bytes, d_status, st); }
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(new_frame, new_idx_off, 1, new_idx_crc, idx_bytes, st); }
    sqzk::launch_frame_seal(new_frame, new_idx_crc, n_blocks, d_status, st, (uint32_t)record);
    { SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
      const uint64_t payload_off = frame_payload_off(n_blocks, record);
      sqzk::launch_frame_splice(frame, slabs, slots, new_frame, seg_dst, seg_src, seg_len, m,
                                capacity > payload_off ? capacity - payload_off : 0, st); }
    return hip_errno(hipGetLastError());
}

int sqz_hip_frame_update(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                         uint32_t win_bits, uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length,
                         uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks, const void* d_data,
                         uint64_t data_bytes, uint64_t* d_data_off, uint32_t parse, void* d_new_frame, uint64_t capacity,
                         uint64_t* d_frame_bytes, int32_t* d_range_err, uint32_t* d_blocks_encoded, int32_t* d_status,
                         void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return frame_update_call(d_frame, avail, n_blocks, content_bytes, win_bits, block_bits, d_offset, d_length, n_ranges,
                             max_length, max_blocks, d_data, data_bytes, d_data_off, parse, NULL, 0, d_new_frame, capacity,
                             d_frame_bytes, d_range_err, d_blocks_encoded, d_status, d_scratch, scratch_bytes, stream);
}

int sqz_hip_frame_update_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                              uint32_t win_bits, uint32_t block_bits, const uint64_t* d_offset, const uint64_t* d_length,
                              uint32_t n_ranges, uint64_t max_length, uint32_t max_blocks, const void* d_data,
                              uint64_t data_bytes, uint64_t* d_data_off, uint32_t parse, const void* d_dict,
                              uint64_t dict_bytes, void* d_new_frame, uint64_t capacity, uint64_t* d_frame_bytes,
                              int32_t* d_range_err, uint32_t* d_blocks_encoded, int32_t* d_status, void* d_scratch,
                              uint64_t scratch_bytes, void* stream) {
    if (win_bits > (uint32_t)sqz_max_win_bits || !dict_ok(d_dict, dict_bytes, 1u << win_bits)) { return EINVAL; }
    return frame_update_call(d_frame, avail, n_blocks, content_bytes, win_bits, block_bits, d_offset, d_length, n_ranges,
                             max_length, max_blocks, d_data, data_bytes, d_data_off, parse, d_dict, dict_bytes, d_new_frame,
                             capacity, d_frame_bytes, d_range_err, d_blocks_encoded, d_status, d_scratch, scratch_bytes,
                             stream);
}

// ---- more content behind a resident frame in one call
// What the host works out for an append from the header's copy: t, the bytes of a ragged last block; whether that block
// is touched; keep, the blocks carried over; m, the blocks to encode; stage = t + data_bytes (t = 0 unless touched).
struct AppendShape { uint64_t tail, keep, m, n_new, stage; bool touched, ok; };
static AppendShape append_shape(uint64_t n_blocks, uint64_t content_bytes, uint64_t data_bytes, uint32_t block_bits) {
    AppendShape S = {};
    const uint64_t bb = 1ull << block_bits;
    S.tail = content_bytes & (bb - 1);
    S.touched = n_blocks > 0 && S.tail != 0 && data_bytes > 0;
    S.keep = n_blocks - (S.touched ? 1 : 0);
    const uint64_t head = S.touched ? S.tail : 0;
    S.ok = data_bytes <= ~content_bytes && data_bytes <= ~(uint64_t)0 - 2 * bb;     // C + A and t + A + 2^b without a wrap
    if (!S.ok) { return S; }
    S.stage = data_bytes > 0 ? head + data_bytes : 0;
    S.m = (S.stage + bb - 1) >> block_bits;
    S.n_new = S.keep + S.m;
    S.ok = S.n_new <= 0xFFFFFFFFull && S.m < 0xFFFFFFFFull;      // n' and the m + 1 segments in 32 bits
    return S;
}

// where the pieces of an append's scratch lie (every piece 256-byte aligned): the open for a list of one block, the
// staging area, what the encode of the m blocks and the new index take.  The encoder's scratch lies over the decoder's.
struct AppendScratch {
    uint64_t bitmap, wpre, misc, sel, in_off, out_off, skip, stored, crc, err, staging, enc_in_off, slab_off, out_bytes,
             enc_err, crc_new, seg_dst, seg_src, seg_len, verdict, dict_idx, slabs, codec, codec_bytes, enc_codec_bytes, total;
};
static AppendScratch append_scratch(uint64_t n, const AppendShape& S, uint32_t block_bits, uint64_t dict_bytes) {
    AppendScratch P = {};
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) { const uint64_t v = at; at += align_up(bytes, 256); return v; };
    const uint64_t words = (n + 31) / 32, m = S.m, bb = 1ull << block_bits;
    P.bitmap = take(words * 4 + 4);
    P.wpre = take(words * 4 + 4);
    P.misc = take(256);                 // as a gather's: [160,168) count and verdict on the request
    P.sel = take(8);
    P.in_off = take(3 * 8);             // one slot, two entries (frame_open_body<.., true>)
    P.out_off = take(3 * 8);
    P.skip = take(2 * 4 + 4);
    P.stored = take(2 * 4 + 4);
    P.crc = take(2 * 4 + 4);
    P.err = take(2 * 4 + 4);
    P.staging = take(S.stage + 16);
    P.enc_in_off = take((m + 1) * 8);
    P.slab_off = take((m + 1) * 8);
    P.out_bytes = take(m * 8 + 8);
    P.enc_err = take(m * 4 + 4);
    P.crc_new = take(m * 4 + 4);
    P.seg_dst = take((m + 2) * 8);
    P.seg_src = take((m + 1) * 8);
    P.seg_len = take((m + 1) * 8);
    P.verdict = take(256);
    P.dict_idx = take(dict_bytes != 0 ? dict_index_bytes(dict_bytes) : 0);
    P.slabs = take(m * sqz_bound(bb));
    P.enc_codec_bytes = sqz_hip_encode_scratch_bytes((uint32_t)m, m << block_bits);
    const uint64_t dec = sqz_hip_decode_scratch_bytes(2, bb);
    P.codec_bytes = dec > P.enc_codec_bytes ? dec : P.enc_codec_bytes;
    P.codec = take(P.codec_bytes);
    P.total = at;
    return P;
}

uint64_t sqz_hip_frame_append_scratch_bytes(uint32_t n_blocks, uint64_t content_bytes, uint64_t data_bytes,
                                            uint32_t block_bits, uint64_t dict_bytes) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        dict_bytes > (uint64_t)sqzk_max_window - 1) { return 0; }
    const AppendShape S = append_shape(n_blocks, content_bytes, data_bytes, block_bits);
    if (!S.ok) { return 0; }
    return append_scratch(n_blocks, S, block_bits, dict_bytes).total;
}

// dict == NULL: versions 1 and 2 (sqz_hip_frame_append); else version 3
static int frame_append_call(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                             uint32_t win_bits, uint32_t block_bits, const void* d_data, uint64_t data_bytes,
                             uint32_t parse, const void* d_dict, uint64_t dict_bytes, void* d_new_frame,
                             uint64_t capacity, uint64_t* d_frame_bytes, uint32_t* d_blocks_encoded, int32_t* d_status,
                             void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!frame_params_ok(win_bits, block_bits) || frame_blocks(content_bytes, block_bits) != n_blocks ||
        !parse_ok(parse)) { return EINVAL; }
    if (d_frame == NULL || ((uintptr_t)d_frame & 15u) != 0 || d_scratch == NULL || ((uintptr_t)d_scratch & 15u) != 0 ||
        d_new_frame == NULL || ((uintptr_t)d_new_frame & 15u) != 0 || d_frame_bytes == NULL ||
        d_status == NULL || d_blocks_encoded == NULL || (data_bytes > 0 && d_data == NULL)) { return EINVAL; }
    const AppendShape S = append_shape(n_blocks, content_bytes, data_bytes, block_bits);
    if (!S.ok || sqz_frame_bound(content_bytes + data_bytes, block_bits) == 0) { return EINVAL; }
    const AppendScratch P = append_scratch(n_blocks, S, block_bits, d_dict != NULL ? dict_bytes : 0);
    if (scratch_bytes < P.total) { return EINVAL; }
    if (spans_overlap(d_new_frame, capacity, d_frame, avail) || spans_overlap(d_new_frame, capacity, d_data, data_bytes) ||
        spans_overlap(d_new_frame, capacity, d_scratch, scratch_bytes) ||
        spans_overlap(d_data, data_bytes, d_scratch, scratch_bytes)) { return EINVAL; }
    const uint64_t record = d_dict != NULL ? 8 : 0;
    if (avail < 32 + 8 * (uint64_t)n_blocks + record) { return E2BIG; }
    const int e = device_ready();
    if (e != 0) { return e; }
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* const frame = (const uint8_t*)d_frame;
    uint8_t* const new_frame = (uint8_t*)d_new_frame;
    uint8_t* const scratch = (uint8_t*)d_scratch;
    uint32_t* bitmap = (uint32_t*)(scratch + P.bitmap);
    uint32_t* wpre = (uint32_t*)(scratch + P.wpre);
    uint64_t* idx_off = (uint64_t*)(scratch + P.misc);
    uint32_t* idx_crc = (uint32_t*)(scratch + P.misc + 16);
    uint64_t* spare = (uint64_t*)(scratch + P.misc + 32);
    uint32_t* ctl = (uint32_t*)(scratch + P.misc + 160);      // [160,168): count, verdict on the request
    uint32_t* sel = (uint32_t*)(scratch + P.sel);
    uint64_t* in_off = (uint64_t*)(scratch + P.in_off);
    uint64_t* out_off = (uint64_t*)(scratch + P.out_off);
    uint32_t* skip = (uint32_t*)(scratch + P.skip);
    uint32_t* stored = (uint32_t*)(scratch + P.stored);
    uint32_t* crc = (uint32_t*)(scratch + P.crc);
    int32_t* err = (int32_t*)(scratch + P.err);
    uint8_t* staging = scratch + P.staging;
    uint64_t* enc_in_off = (uint64_t*)(scratch + P.enc_in_off);
    uint64_t* slab_off = (uint64_t*)(scratch + P.slab_off);
    uint64_t* out_bytes = (uint64_t*)(scratch + P.out_bytes);
    int32_t* enc_err = (int32_t*)(scratch + P.enc_err);
    uint32_t* crc_new = (uint32_t*)(scratch + P.crc_new);
    uint64_t* seg_dst = (uint64_t*)(scratch + P.seg_dst);
    uint64_t* seg_src = (uint64_t*)(scratch + P.seg_src);
    uint64_t* seg_len = (uint64_t*)(scratch + P.seg_len);
    uint64_t* new_idx_off = (uint64_t*)(scratch + P.verdict + 16);       // the verdict words: [16,32) the new index's
    uint32_t* new_idx_crc = (uint32_t*)(scratch + P.verdict + 32);       // range, [32,36) its checksum, [64,104) the
    uint64_t* copy = (uint64_t*)(scratch + P.verdict + 64);              // staging copy's work list
    uint8_t* slabs = scratch + P.slabs;
    const uint64_t bb = 1ull << block_bits, slab = sqz_bound(bb);
    const uint32_t m = (uint32_t)S.m, n_new = (uint32_t)S.n_new;
    // the last block as a list of one, if it is touched, and the verdict on the request
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_append_plan(frame, n_blocks, content_bytes, data_bytes, block_bits, win_bits, bitmap, wpre, sel, ctl, st); }
    // the frame's checks and the touched block to the head of the staging area, as a gather's into its slot
    const uint64_t idx_bytes = 8 * (uint64_t)n_blocks + record;
    sqzk::launch_frame_plan(1, idx_bytes, idx_bytes, 0, idx_off, spare, st);
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(frame + 32, idx_off, 1, idx_crc, idx_bytes, st); }
    DictDev dd;
    uint32_t* dict_crc = nullptr;
    if (d_dict != NULL) {
        uint64_t* dict_off = (uint64_t*)(scratch + P.misc + 64);
        dict_crc = (uint32_t*)(scratch + P.misc + 128);
        sqzk::launch_frame_plan(1, dict_bytes, dict_bytes, 0, dict_off, dict_off + 4, st);
        SpanGuard g(st, SQZ_HIP_K_CRC32);
        sqzk::launch_crc32_blocks((const uint8_t*)d_dict, dict_off, 1, dict_crc, dict_bytes, st);
        dd.bytes = (const uint8_t*)d_dict; dd.len = (uint32_t)dict_bytes;
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_frame_open_list(frame, avail, n_blocks, content_bytes, idx_crc, (uint32_t)dict_bytes, dict_crc, bitmap,
                                   wpre, sel, ctl, 1, in_off, out_off, skip, stored, d_status, d_blocks_encoded, st,
                                   block_bits); }
    if (S.touched) {
        uint32_t* counts = (uint32_t*)(scratch + P.codec);
        uint32_t* tokens = (uint32_t*)(scratch + P.codec + 256);
        run_frame_decode(frame, in_off, out_off, 2, bb, tokens, counts, staging, err, skip, stored, crc, dd, st, 1);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_append_verdict(frame, n_blocks, ctl, err, crc, block_bits, content_bytes, data_bytes, m, slab, d_status,
                                  d_blocks_encoded, copy, enc_in_off, slab_off, st); }
    if (m > 0) {
        { SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);                // the data behind the touched block's bytes
          sqzk::launch_range_copy((const uint8_t*)d_data, copy, staging, copy + 1, copy + 2, (const uint32_t*)(copy + 4), 1,
                                  false, data_bytes, st); }
        { SpanGuard g(st, SQZ_HIP_K_CRC32);
          sqzk::launch_crc32_blocks(staging, enc_in_off, m, crc_new, bb, st); }
        if (d_dict != NULL) { dd = run_dict_index((const uint8_t*)d_dict, (uint32_t)dict_bytes, scratch + P.dict_idx, st); }
        const uint64_t head = align_up((uint64_t)m * 4, 256);
        const uint64_t slots_n = (P.enc_codec_bytes - head) / 8;
        uint32_t* counts = (uint32_t*)(scratch + P.codec);
        uint32_t* tokens = (uint32_t*)(scratch + P.codec + head);
        run_encode(d_dict != NULL ? 1 : finder_for(parse), staging, enc_in_off, m, 1u << win_bits, tokens, counts, tokens,
                   tokens + slots_n, bb, slabs, slab_off, out_bytes, enc_err, 0, 0, slots_n, nullptr, st, parse,
                   d_dict != NULL ? &dd : nullptr);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      sqzk::launch_frame_append_index(frame, n_blocks, content_bytes, data_bytes, m, d_dict != NULL, out_bytes, enc_err,
                                      crc_new, slab, new_frame, capacity, seg_dst, seg_src, seg_len, new_idx_off,
                                      d_frame_bytes, d_status, st); }
    const uint64_t new_idx_bytes = 8 * (uint64_t)n_new + record;
    { SpanGuard g(st, SQZ_HIP_K_CRC32);
      sqzk::launch_crc32_blocks(new_frame, new_idx_off, 1, new_idx_crc, new_idx_bytes, st); }
    sqzk::launch_frame_seal(new_frame, new_idx_crc, n_new, d_status, st, (uint32_t)record);
    { SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
      const uint64_t payload_off = frame_payload_off(n_new, record);
      sqzk::launch_frame_splice_segments(frame, slabs, staging, new_frame, seg_dst, seg_src, seg_len, m + 1,
                                         capacity > payload_off ? capacity - payload_off : 0, st); }
    return hip_errno(hipGetLastError());
}

int sqz_hip_frame_append(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                         uint32_t win_bits, uint32_t block_bits, const void* d_data, uint64_t data_bytes,
                         uint32_t parse, void* d_new_frame, uint64_t capacity, uint64_t* d_frame_bytes,
                         uint32_t* d_blocks_encoded, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                         void* stream) {
    return frame_append_call(d_frame, avail, n_blocks, content_bytes, win_bits, block_bits, d_data, data_bytes, parse,
                             NULL, 0, d_new_frame, capacity, d_frame_bytes, d_blocks_encoded, d_status, d_scratch,
                             scratch_bytes, stream);
}

int sqz_hip_frame_append_dict(const void* d_frame, uint64_t avail, uint32_t n_blocks, uint64_t content_bytes,
                              uint32_t win_bits, uint32_t block_bits, const void* d_data, uint64_t data_bytes,
                              uint32_t parse, const void* d_dict, uint64_t dict_bytes, void* d_new_frame,
                              uint64_t capacity, uint64_t* d_frame_bytes, uint32_t* d_blocks_encoded, int32_t* d_status,
                              void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (win_bits > (uint32_t)sqz_max_win_bits || !dict_ok(d_dict, dict_bytes, 1u << win_bits)) { return EINVAL; }
    return frame_append_call(d_frame, avail, n_blocks, content_bytes, win_bits, block_bits, d_data, data_bytes, parse,
                             d_dict, dict_bytes, d_new_frame, capacity, d_frame_bytes, d_blocks_encoded, d_status,
                             d_scratch, scratch_bytes, stream);
}

// ---- many frames in one call ("Batches of frames")
// what the host works out from the k sizes of an encode: total blocks, total content, frame_at[k]; !ok: a size wraps,
// or blocks + k does not fit 31 bits
struct FramesEncShape { uint64_t blocks, content, bound; bool ok; };
static FramesEncShape frames_enc_shape(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits, uint32_t flags,
                                       uint64_t* frame_at, const uint32_t* elem_bytes = nullptr) {
    // elem_bytes (null: none): a frame with an element size takes sqz_frame_bound_shuf's room
    FramesEncShape S = {0, 0, 0, false};
    for (uint32_t f = 0; f < k; f++) {
        const uint64_t c = content_bytes[f];
        if (c > (1ull << 62)) { return S; }                     // twice the content and more: the bound would wrap
        const uint64_t slot = align_up(elem_bytes != nullptr && elem_bytes[f] != 0
                                           ? sqz_frame_bound_shuf(c, block_bits, flags | (uint32_t)SQZ_FRAME_SHUFFLE)
                                           : sqz_frame_bound_ex(c, block_bits, flags), 16);
        if (frame_at != NULL) { frame_at[f] = S.bound; }
        if (slot == 0 || S.bound > ~slot || S.content > ~c) { return S; }
        S.bound += slot;
        S.content += c;
        S.blocks += frame_blocks(c, block_bits);
        if (S.blocks + k > 0x7FFFFFFFull) { return S; }
    }
    if (frame_at != NULL) { frame_at[k] = S.bound; }
    S.ok = true;
    return S;
}

struct FramesEncScratch {
    uint64_t content, in_at, frame_at, base, in_off, slab_off, crc, out_bytes, copy_bytes, dense_rel, dense_off, stored,
             slabs, codec, codec_bytes, elem, blk_elem, shuf, total;
};
// shuf: a batch with shuffled frames keeps, behind everything else, the k element sizes, one per block of the batch, and
// the whole content as the encoder reads it
static FramesEncScratch frames_enc_scratch(uint64_t k, uint64_t n, uint64_t content_bytes, uint64_t slab_bytes, bool store,
                                           bool shuf = false) {
    FramesEncScratch L = {};
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) { const uint64_t r = at; at += align_up(bytes, 256); return r; };
    L.content = take(k * 8);
    L.in_at = take((k + 1) * 8);
    L.frame_at = take((k + 1) * 8);
    L.base = take((k + 1) * 4);
    L.in_off = take((n + 1) * 8);
    L.slab_off = take((n + 1) * 8);
    L.crc = take(n * 4 + 4);
    L.out_bytes = take(n * 8);
    L.copy_bytes = take(n * 8);
    L.dense_rel = take((n + k) * 8);
    L.dense_off = take((n + 1) * 8);
    L.stored = store ? take(n * 4 + 4) : 0;
    L.slabs = take(n * slab_bytes);
    L.codec_bytes = sqz_hip_encode_scratch_bytes((uint32_t)n, content_bytes);
    L.codec = take(L.codec_bytes);
    if (shuf) {
        L.elem = take(k * 4);
        L.blk_elem = take(n * 4 + 4);
        L.shuf = take(content_bytes + 16);
    }
    L.total = at;
    return L;
}

uint64_t sqz_hip_frames_bound(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits, uint32_t flags,
                              uint64_t* frame_at) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        !frame_flags_ok(flags) || (content_bytes == NULL && k > 0)) { return 0; }
    const FramesEncShape S = frames_enc_shape(content_bytes, k, block_bits, flags, frame_at);
    return S.ok ? S.bound : 0;
}

uint64_t sqz_hip_frames_encode_scratch_bytes(const uint64_t* content_bytes, uint32_t k, uint32_t block_bits,
                                             uint32_t flags) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        !frame_flags_ok(flags) || (content_bytes == NULL && k > 0)) { return 0; }
    const FramesEncShape S = frames_enc_shape(content_bytes, k, block_bits, flags, NULL);
    if (!S.ok) { return 0; }
    return frames_enc_scratch(k, S.blocks, S.content, sqz_bound(1ull << block_bits), (flags & SQZ_FRAME_STORED) != 0).total;
}

// elem_bytes: null for the call there always was; else k element sizes, one of them not 0 (sqz_hip_frames_encode_shuf)
static int frames_encode_call(const void* d_in, const uint64_t* content_bytes, const uint32_t* elem_bytes, uint32_t k,
                              uint32_t win_bits, uint32_t block_bits, uint32_t flags, uint32_t parse, void* d_frames,
                              uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err,
                              void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!parse_ok(parse) || !frame_flags_ok(flags) || !frame_params_ok(win_bits, block_bits)) { return EINVAL; }
    if (k == 0) { return 0; }
    if (content_bytes == NULL || d_frames == NULL || ((uintptr_t)d_frames & 15u) != 0 || d_frame_bytes == NULL ||
        d_status == NULL || d_scratch == NULL || ((uintptr_t)d_scratch & 15u) != 0) { return EINVAL; }
    const bool shuf = elem_bytes != nullptr;
    const FramesEncShape S = frames_enc_shape(content_bytes, k, block_bits, flags, NULL, elem_bytes);
    if (!S.ok || (d_in == NULL && S.content > 0) || (d_err == NULL && S.blocks > 0) || capacity < S.bound) { return EINVAL; }
    const uint64_t bb = 1ull << block_bits, slab = sqz_bound(bb);
    const bool store = (flags & SQZ_FRAME_STORED) != 0;
    const uint32_t n = (uint32_t)S.blocks;
    const FramesEncScratch L = frames_enc_scratch(k, n, S.content, slab, store, shuf);
    if (scratch_bytes < L.total) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    hipStream_t st = (hipStream_t)stream;
    uint8_t* const scratch = (uint8_t*)d_scratch;
    uint64_t* sizes = (uint64_t*)(scratch + L.content);
    uint64_t* in_at = (uint64_t*)(scratch + L.in_at);
    uint64_t* frame_at = (uint64_t*)(scratch + L.frame_at);
    uint32_t* base = (uint32_t*)(scratch + L.base);
    uint64_t* in_off = (uint64_t*)(scratch + L.in_off);
    uint64_t* slab_off = (uint64_t*)(scratch + L.slab_off);
    uint32_t* crc = (uint32_t*)(scratch + L.crc);
    uint64_t* out_bytes = (uint64_t*)(scratch + L.out_bytes);
    uint64_t* copy_bytes = (uint64_t*)(scratch + L.copy_bytes);
    uint64_t* dense_rel = (uint64_t*)(scratch + L.dense_rel);
    uint64_t* dense_off = (uint64_t*)(scratch + L.dense_off);
    uint32_t* stored = store ? (uint32_t*)(scratch + L.stored) : nullptr;
    uint32_t* elem = shuf ? (uint32_t*)(scratch + L.elem) : nullptr;
    uint32_t* blk_elem = shuf ? (uint32_t*)(scratch + L.blk_elem) : nullptr;
    HIP_TRY(hipMemcpyAsync(sizes, content_bytes, (size_t)k * 8, hipMemcpyHostToDevice, st));
    if (shuf) {
        HIP_TRY(hipMemcpyAsync(elem, elem_bytes, (size_t)k * 4, hipMemcpyHostToDevice, st));
        sqzk::launch_frames_encode_scan_v4(sizes, elem, k, block_bits, flags, in_at, frame_at, base, st);
        sqzk::launch_frames_plan_v4(sizes, elem, in_at, base, k, block_bits, slab, in_off, slab_off, blk_elem, st);
    } else {
        sqzk::launch_frames_encode_scan(sizes, k, block_bits, flags, in_at, frame_at, base, st);
        sqzk::launch_frames_plan(sizes, in_at, base, k, block_bits, slab, in_off, slab_off, st);
    }
    if (n > 0) {
        { SpanGuard g(st, SQZ_HIP_K_CRC32);
          sqzk::launch_crc32_blocks((const uint8_t*)d_in, in_off, n, crc, bb, st); }
        const uint64_t head = align_up((uint64_t)n * 4, 256);
        const uint64_t slots = (L.codec_bytes - head) / 8;
        uint32_t* counts = (uint32_t*)(scratch + L.codec);
        uint32_t* tokens = (uint32_t*)(scratch + L.codec + head);
        const uint8_t* enc_in = (const uint8_t*)d_in;       // shuffled frames: the encoder reads the whole batch from the
        if (shuf) {                                         // scratch, every block shuffled by its frame's element size or
            sqzk::launch_shuffle_ranges((const uint8_t*)d_in, in_off, blk_elem, n, false, scratch + L.shuf, nullptr, bb,
                                        st);                // copied; checksums (above) and stored blocks (below) keep to
            enc_in = scratch + L.shuf;                      // the caller's bytes
        }
        run_encode(finder_for(parse), enc_in, in_off, n, 1u << win_bits, tokens, counts, tokens,
                   tokens + slots, bb, scratch + L.slabs, slab_off, out_bytes, d_err, 0, 0, slots, nullptr, st, parse);
    }
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      if (shuf) {
          sqzk::launch_frames_index_v4(out_bytes, d_err, crc, sizes, elem, frame_at, base, k, win_bits, block_bits, flags,
                                       (uint8_t*)d_frames, copy_bytes, dense_rel, dense_off, stored, d_frame_bytes,
                                       d_status, st);
      } else {
          sqzk::launch_frames_index(out_bytes, d_err, crc, sizes, frame_at, base, k, win_bits, block_bits, flags,
                                    (uint8_t*)d_frames, copy_bytes, dense_rel, dense_off, stored, d_frame_bytes, d_status,
                                    st);
      } }
    if (n > 0) {
        sqzk::launch_compact_blocks(scratch + L.slabs, slab_off, copy_bytes, n, (uint8_t*)d_frames, dense_off, bb / 2, st);
        if (store) {                                        // the stored blocks' content, where the indexes say
            SpanGuard g(st, SQZ_HIP_K_RANGE_COPY);
            sqzk::launch_range_copy((const uint8_t*)d_in, in_off, (uint8_t*)d_frames, dense_off, in_off, stored, n, true,
                                    bb, st);
        }
    }
    return hip_errno(hipGetLastError());
}

int sqz_hip_frames_encode(const void* d_in, const uint64_t* content_bytes, uint32_t k, uint32_t win_bits,
                          uint32_t block_bits, uint32_t flags, uint32_t parse, void* d_frames, uint64_t capacity,
                          uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err, void* d_scratch,
                          uint64_t scratch_bytes, void* stream) {
    return frames_encode_call(d_in, content_bytes, nullptr, k, win_bits, block_bits, flags, parse, d_frames, capacity,
                              d_frame_bytes, d_status, d_err, d_scratch, scratch_bytes, stream);
}

// ---- batches that know version 4: one element size per frame, 0 for a frame that is not shuffled
// 0: every one of the k values is 0 (the calls there always were do the work); 1: one at least is 2, 4 or 8;
// -1: a value that is none of these, or no array
static int frames_elem_kind(const uint32_t* elem_bytes, uint32_t k) {
    if (elem_bytes == NULL) { return k == 0 ? 0 : -1; }
    int kind = 0;
    for (uint32_t f = 0; f < k; f++) {
        if (elem_bytes[f] != 0) {
            if (!elem_ok(elem_bytes[f])) { return -1; }
            kind = 1;
        }
    }
    return kind;
}

uint64_t sqz_hip_frames_bound_shuf(const uint64_t* content_bytes, const uint32_t* elem_bytes, uint32_t k,
                                   uint32_t block_bits, uint32_t flags, uint64_t* frame_at) {
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        !frame_flags_ok(flags) || (content_bytes == NULL && k > 0) || frames_elem_kind(elem_bytes, k) < 0) { return 0; }
    const FramesEncShape S = frames_enc_shape(content_bytes, k, block_bits, flags, frame_at, elem_bytes);
    return S.ok ? S.bound : 0;
}

uint64_t sqz_hip_frames_encode_scratch_bytes_shuf(const uint64_t* content_bytes, const uint32_t* elem_bytes, uint32_t k,
                                                  uint32_t block_bits, uint32_t flags) {
    const int kind = frames_elem_kind(elem_bytes, k);
    if (kind < 0) { return 0; }
    if (kind == 0) { return sqz_hip_frames_encode_scratch_bytes(content_bytes, k, block_bits, flags); }
    if (block_bits < (uint32_t)sqz_frame_min_block_bits || block_bits > (uint32_t)sqz_frame_max_block_bits ||
        !frame_flags_ok(flags) || content_bytes == NULL) { return 0; }
    const FramesEncShape S = frames_enc_shape(content_bytes, k, block_bits, flags, NULL, elem_bytes);
    if (!S.ok) { return 0; }
    return frames_enc_scratch(k, S.blocks, S.content, sqz_bound(1ull << block_bits), (flags & SQZ_FRAME_STORED) != 0,
                              true).total;
}

int sqz_hip_frames_encode_shuf(const void* d_in, const uint64_t* content_bytes, const uint32_t* elem_bytes, uint32_t k,
                               uint32_t win_bits, uint32_t block_bits, uint32_t flags, uint32_t parse, void* d_frames,
                               uint64_t capacity, uint64_t* d_frame_bytes, int32_t* d_status, int32_t* d_err,
                               void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!parse_ok(parse) || !frame_flags_ok(flags) || !frame_params_ok(win_bits, block_bits)) { return EINVAL; }
    if (k == 0) { return 0; }
    const int kind = frames_elem_kind(elem_bytes, k);
    if (kind < 0) { return EINVAL; }
    // no frame is shuffled: exactly what sqz_hip_frames_encode enqueues, no pass and no scratch for one
    return frames_encode_call(d_in, content_bytes, kind == 0 ? nullptr : elem_bytes, k, win_bits, block_bits, flags,
                              parse, d_frames, capacity, d_frame_bytes, d_status, d_err, d_scratch, scratch_bytes, stream);
}

// what the host works out from the table of a decode: total blocks, the span of the outputs, the largest block's size
// as far as the table says (it only sizes launches); err: EINVAL / E2BIG as the call answers them
// shuf (the _shuf calls): the last word of an item is the frame's element size, 0, 2, 4 or 8, and any: one is not 0
struct FramesDecShape { uint64_t blocks, extent, hint; int err; bool any; };
static FramesDecShape frames_dec_shape(const struct sqz_frames_item* items, uint32_t k, bool shuf = false) {
    FramesDecShape S = {0, 0, 1, 0, false};
    for (uint32_t f = 0; f < k; f++) {
        const struct sqz_frames_item& it = items[f];
        if (it.zero != 0) { S.any = true; }
        if ((it.frame_at & 15u) != 0 || (shuf ? it.zero != 0 && !elem_ok(it.zero) : it.zero != 0) ||
            it.avail > ~it.frame_at || it.content_bytes > ~it.out_at) {
            S.err = EINVAL;
            return S;
        }
        if (f + 1 < k && (it.frame_at + it.avail > items[f + 1].frame_at ||
                          it.out_at + it.content_bytes > items[f + 1].out_at)) { S.err = EINVAL; return S; }
        S.blocks += it.n_blocks;
        if (S.blocks + k > 0x7FFFFFFFull) { S.err = EINVAL; return S; }
        if (it.n_blocks > 0) {
            const uint64_t per = (it.content_bytes + it.n_blocks - 1) / it.n_blocks;
            if (per > S.hint) { S.hint = per; }
        }
    }
    if (k > 0) { S.extent = items[k - 1].out_at + items[k - 1].content_bytes - items[0].out_at; }
    if (S.extent > (1ull << 60)) { S.err = EINVAL; return S; }     // four bytes of scratch per byte of it
    for (uint32_t f = 0; f < k; f++) {
        if (items[f].avail < 32 + 8 * (uint64_t)items[f].n_blocks + (items[f].zero != 0 ? 8 : 0)) { S.err = E2BIG; return S; }
    }
    return S;
}

struct FramesDecScratch {
    uint64_t items, base, in_off, out_off, skip, stored, crc, err, codec, codec_bytes, ent_elem, shuf, total;
};
// shuf: a batch with shuffled frames keeps, behind everything else, one element size per entry and the span of the
// outputs once more, as the decoder leaves it
static FramesDecScratch frames_dec_scratch(uint64_t k, uint64_t entries, uint64_t extent, bool shuf = false) {
    FramesDecScratch L = {};
    uint64_t at = 0;
    auto take = [&at](uint64_t bytes) { const uint64_t r = at; at += align_up(bytes, 256); return r; };
    L.items = take(k * sizeof(struct sqz_frames_item));
    L.base = take((k + 1) * 4);
    L.in_off = take((entries + 1) * 8);
    L.out_off = take((entries + 1) * 8);
    L.skip = take(entries * 4 + 4);
    L.stored = take(entries * 4 + 4);
    L.crc = take(entries * 4 + 4);
    L.err = take(entries * 4 + 4);
    L.codec_bytes = sqz_hip_decode_scratch_bytes((uint32_t)entries, extent);
    L.codec = take(L.codec_bytes);
    if (shuf) {
        L.ent_elem = take(entries * 4 + 4);
        L.shuf = take(extent + 16);
    }
    L.total = at;
    return L;
}
static_assert(sizeof(struct sqz_frames_item) == 40, "the table of a batched decode: 40 bytes per frame (sqz.h)");

uint64_t sqz_hip_frames_decode_scratch_bytes(const struct sqz_frames_item* items, uint32_t k) {
    if (items == NULL && k > 0) { return 0; }
    const FramesDecShape S = frames_dec_shape(items, k);
    return S.err != 0 ? 0 : frames_dec_scratch(k, S.blocks + k, S.extent).total;
}

// with_elem: sqz_hip_frames_decode_shuf, where an item's last word is the frame's element size
static int frames_decode_call(const void* d_frames, const struct sqz_frames_item* items, uint32_t k, void* d_out,
                              int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream,
                              bool with_elem) {
    if (k == 0) { return 0; }
    if (items == NULL || d_frames == NULL || ((uintptr_t)d_frames & 15u) != 0 || d_status == NULL || d_scratch == NULL ||
        ((uintptr_t)d_scratch & 15u) != 0) { return EINVAL; }
    const FramesDecShape S = frames_dec_shape(items, k, with_elem);
    if (S.err == EINVAL || (S.blocks > 0 && (d_out == NULL || d_err == NULL))) { return EINVAL; }
    const uint32_t n = (uint32_t)S.blocks, entries = n + k;
    const bool shuf = with_elem && S.any;                   // no element size named: what there always was
    const FramesDecScratch L = frames_dec_scratch(k, entries, S.extent, shuf);
    if (scratch_bytes < L.total) { return EINVAL; }
    if (S.err != 0) { return S.err; }
    const int e = device_ready();
    if (e != 0) { return e; }
    hipStream_t st = (hipStream_t)stream;
    uint8_t* const scratch = (uint8_t*)d_scratch;
    struct sqz_frames_item* table = (struct sqz_frames_item*)(scratch + L.items);
    uint32_t* base = (uint32_t*)(scratch + L.base);
    uint64_t* in_off = (uint64_t*)(scratch + L.in_off);
    uint64_t* out_off = (uint64_t*)(scratch + L.out_off);
    uint32_t* skip = (uint32_t*)(scratch + L.skip);
    uint32_t* stored = (uint32_t*)(scratch + L.stored);
    uint32_t* crc = (uint32_t*)(scratch + L.crc);
    int32_t* err = (int32_t*)(scratch + L.err);
    const uint64_t out_base = items[0].out_at;
    HIP_TRY(hipMemcpyAsync(table, items, (size_t)k * sizeof(struct sqz_frames_item), hipMemcpyHostToDevice, st));
    sqzk::launch_frames_decode_scan(table, k, base, st);
    uint32_t* ent_elem = shuf ? (uint32_t*)(scratch + L.ent_elem) : nullptr;
    { SpanGuard g(st, SQZ_HIP_K_FRAME_INDEX);
      if (shuf) {
          sqzk::launch_frames_open_v4((const uint8_t*)d_frames, table, base, k, out_base, in_off, out_off, skip, stored,
                                      ent_elem, d_status, st);
      } else {
          sqzk::launch_frames_open((const uint8_t*)d_frames, table, base, k, out_base, in_off, out_off, skip, stored,
                                   d_status, st);
      } }
    if (n > 0) {
        uint32_t* counts = (uint32_t*)(scratch + L.codec);
        uint32_t* tokens = (uint32_t*)(scratch + L.codec + align_up((uint64_t)entries * 4, 256));
        // shuffled frames: the expansion writes the whole span into the scratch, the inverse pass brings every block
        // that is not stored to d_out, shuffled back by its frame's element size or copied
        run_frame_decode((const uint8_t*)d_frames, in_off, out_off, entries, S.hint, tokens, counts,
                         (uint8_t*)d_out + out_base, err, skip, stored, crc, DictDev(), st, n,
                         shuf ? scratch + L.shuf : nullptr, 0, ent_elem);
        sqzk::launch_frames_verify((const uint8_t*)d_frames, table, base, k, crc, d_status, err, d_err, st);
    }
    return hip_errno(hipGetLastError());
}

int sqz_hip_frames_decode(const void* d_frames, const struct sqz_frames_item* items, uint32_t k, void* d_out,
                          int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return frames_decode_call(d_frames, items, k, d_out, d_err, d_status, d_scratch, scratch_bytes, stream, false);
}

uint64_t sqz_hip_frames_decode_scratch_bytes_shuf(const struct sqz_frames_item* items, uint32_t k) {
    if (items == NULL && k > 0) { return 0; }
    const FramesDecShape S = frames_dec_shape(items, k, true);
    return S.err != 0 ? 0 : frames_dec_scratch(k, S.blocks + k, S.extent, S.any).total;
}

int sqz_hip_frames_decode_shuf(const void* d_frames, const struct sqz_frames_item* items, uint32_t k, void* d_out,
                               int32_t* d_err, int32_t* d_status, void* d_scratch, uint64_t scratch_bytes,
                               void* stream) {
    return frames_decode_call(d_frames, items, k, d_out, d_err, d_status, d_scratch, scratch_bytes, stream, true);
}

int sqz_hip_shuffle_ranges(const void* d_in, const uint64_t* d_off, const uint32_t* d_elem, uint32_t n, int inverse,
                           void* d_out, const uint32_t* d_skip, void* stream) {
    if (n == 0) { return 0; }
    if (d_in == NULL || d_off == NULL || d_elem == NULL || d_out == NULL || d_in == d_out) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    sqzk::launch_shuffle_ranges((const uint8_t*)d_in, d_off, d_elem, n, inverse != 0, (uint8_t*)d_out, d_skip, 0,
                                (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

int sqz_hip_shuffle_blocks_masked(const void* d_in, const uint64_t* d_off, uint32_t n, uint32_t elem_bytes, int inverse,
                                  void* d_out, const uint32_t* d_mask, void* stream) {
    if (elem_bytes != 0 && !elem_ok(elem_bytes)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (d_in == NULL || d_off == NULL || d_out == NULL || d_mask == NULL || d_in == d_out) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    if (elem_bytes == 0) {
        sqzk::launch_range_copy((const uint8_t*)d_in, d_off, (uint8_t*)d_out, d_off, d_off, d_mask, n, false, 0,
                                (hipStream_t)stream);
    } else {
        sqzk::launch_shuffle_blocks((const uint8_t*)d_in, d_off, n, elem_bytes, inverse != 0, (uint8_t*)d_out, d_mask, 0,
                                    (hipStream_t)stream);
    }
    return hip_errno(hipGetLastError());
}

int sqz_hip_crc32_blocks(const void* d_in, const uint64_t* d_in_off, uint32_t n, uint32_t* d_crc, void* stream) {
    if (n == 0) { return 0; }
    if (d_in == NULL || d_in_off == NULL || d_crc == NULL) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    SpanGuard g((hipStream_t)stream, SQZ_HIP_K_CRC32);
    sqzk::launch_crc32_blocks((const uint8_t*)d_in, d_in_off, n, d_crc, 0, (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

int sqz_hip_shuffle_blocks(const void* d_in, const uint64_t* d_off, uint32_t n, uint32_t elem_bytes, int inverse,
                           void* d_out, void* stream) {
    if (!elem_ok(elem_bytes)) { return EINVAL; }
    if (n == 0) { return 0; }
    if (d_in == NULL || d_off == NULL || d_out == NULL || d_in == d_out) { return EINVAL; }
    const int e = device_ready();
    if (e != 0) { return e; }
    sqzk::launch_shuffle_blocks((const uint8_t*)d_in, d_off, n, elem_bytes, inverse != 0, (uint8_t*)d_out, nullptr, 0,
                                (hipStream_t)stream);
    return hip_errno(hipGetLastError());
}

// ------------------------------------------------------------------ timing
void sqz_hip_set_timing(int enabled) {
    Timing& t = timing();
    std::lock_guard<std::mutex> g(t.mu);
    t.enabled = enabled != 0;
}

int sqz_hip_get_timing(sqz_hip_timing* out, int reset) {
    Timing& t = timing();
    std::lock_guard<std::mutex> g(t.mu);
    t.drain_locked();
    if (out != NULL) { *out = t.acc; }
    if (reset) { t.acc = sqz_hip_timing{}; }
    return 0;
}

} // extern "C"
