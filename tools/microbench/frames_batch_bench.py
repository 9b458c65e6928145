"""What many frames in ONE call buy over one call per frame, in one GPU visit ("Batches of
frames").  Zipf content from sqz_hip_zipf_blocks, window 2^15, through the C ABI on torch's current stream.

  a  64 frames of 1 MiB (four 256 KB blocks each): sqz_hip_frames_encode against 64 sqz_hip_frame_encode_ex calls on
     one stream, and sqz_hip_frames_decode against 64 sqz_hip_frame_decode calls
  b  the same 256 blocks as ONE frame through the single calls: the floor a batch cannot beat
  c  1024 frames of one 4 KB block each against the same 1024 blocks as one frame

The two sides of every comparison leave the same bytes (asserted), alternate `--repeats` times after a warm-up of each,
and every figure is a HIP event pair on the launch stream: median and spread (max - min).

  --trace K   one batched encode and one batched decode of K frames of 1 MiB and nothing else that launches a kernel
              of the library: for `rocprofv3 --kernel-trace --stats -- python ... --trace K`, whose kernel counts for
              K = 1 and K = 64 must be equal (d)
  --trace-one the 256 blocks as one frame through the single calls, for the same kind of run: where a batch's
              distance to (b) goes
  --small     with either: (c)'s shapes instead, K frames of one 4 KB block / 1024 such blocks as one frame
  --layout-probe   (c) once more for the decode alone, with 1, 2, 3, 4 and 7 blocks of 4 KB per frame: how the entries
              that are switched off between the frames' streams show in the decoder's time

    python tools/microbench/frames_batch_bench.py [--out profiles/frames_batch_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WIN_BITS = 15


def stats(xs):
    return {"ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
            "spread_ms": round(max(xs) - min(xs), 4)}


class Shape:
    """k frames of `blocks` blocks of 2^bits bytes each, and everything both sides of a comparison need on the device"""

    def __init__(self, k, blocks, bits):
        import numpy as np
        import torch
        from sqz_amd import _native as N, batch as B, frame as F
        self.torch, self.L, self.k, self.blocks, self.bits = torch, N.lib(), k, blocks, bits
        L = self.L
        self.size = blocks << bits
        self.d_in = B.zipf_blocks(k * blocks, 1 << bits)
        self.sizes = F._pinned(np.full(k, self.size, np.uint64))
        self.total, self.frame_at = F.frames_bound([self.size] * k, bits)
        self.room = self.frame_at[1] if k > 1 else self.total
        z32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
        self.frames = [torch.zeros(self.total + 16, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.frame_bytes = [torch.zeros(k, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.status, self.err = [z32(k), z32(k)], [z32(k * blocks), z32(k * blocks)]
        self.out = [torch.zeros(k * self.size, dtype=torch.uint8, device="cuda") for _ in range(2)]
        need = max(int(L.sqz_hip_frames_encode_scratch_bytes(F._ptr(self.sizes), k, bits, 0)),
                   int(L.sqz_hip_frame_scratch_bytes_ex(self.size, bits, 1, 0)))
        self.scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.items, self.dec_scratch = None, None
        self.F = F

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def check(self, rc):
        assert rc == 0, rc

    def encode_batch(self):
        p = self.F._ptr
        self.check(self.L.sqz_hip_frames_encode(p(self.d_in), p(self.sizes), self.k, WIN_BITS, self.bits, 0, 0,
                                                p(self.frames[0]), self.total, p(self.frame_bytes[0]), p(self.status[0]),
                                                p(self.err[0]), p(self.scratch), self.scratch.numel(), self.stream()))

    def encode_singles(self):
        s = self.stream()
        for f in range(self.k):
            self.check(self.L.sqz_hip_frame_encode_ex(
                self.d_in.data_ptr() + f * self.size, self.size, WIN_BITS, self.bits, 0,
                self.frames[1].data_ptr() + self.frame_at[f], self.room, self.frame_bytes[1].data_ptr() + 8 * f,
                self.status[1].data_ptr() + 4 * f, self.err[1].data_ptr() + 4 * f * self.blocks, self.scratch.data_ptr(),
                self.scratch.numel(), s))

    def prepare_decode(self):
        """after an encode_batch and a synchronise: the table of the decode and its scratch"""
        import numpy as np
        self.sizes_host = self.frame_bytes[0].cpu().tolist()
        assert self.status[0].cpu().tolist() == [0] * self.k
        items = np.zeros(self.k, np.dtype([("frame_at", "<u8"), ("avail", "<u8"), ("content_bytes", "<u8"),
                                           ("out_at", "<u8"), ("n_blocks", "<u4"), ("zero", "<u4")]))
        for f in range(self.k):
            items[f] = (self.frame_at[f], self.sizes_host[f], self.size, f * self.size, self.blocks, 0)
        self.items = self.F._pinned(items)
        need = max(int(self.L.sqz_hip_frames_decode_scratch_bytes(self.F._ptr(self.items), self.k)),
                   int(self.L.sqz_hip_frame_scratch_bytes(self.size, self.bits, 0)))
        assert need > 0
        self.dec_scratch = self.torch.empty(need, dtype=self.torch.uint8, device="cuda")

    def decode_batch(self):
        p = self.F._ptr
        self.check(self.L.sqz_hip_frames_decode(p(self.frames[0]), p(self.items), self.k, p(self.out[0]), p(self.err[0]),
                                                p(self.status[0]), p(self.dec_scratch), self.dec_scratch.numel(),
                                                self.stream()))

    def decode_singles(self):
        s = self.stream()
        for f in range(self.k):
            self.check(self.L.sqz_hip_frame_decode(
                self.frames[0].data_ptr() + self.frame_at[f], self.sizes_host[f], self.blocks, self.size,
                self.out[1].data_ptr() + f * self.size, self.err[1].data_ptr() + 4 * f * self.blocks,
                self.status[1].data_ptr() + 4 * f, self.dec_scratch.data_ptr(), self.dec_scratch.numel(), s))


def timed(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def alternate(torch, sides, repeats):
    for fn in sides.values():                                # a warm-up of either side
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            times[name].append(timed(torch, fn))
    return {name: stats(v) for name, v in times.items()}


def compare(torch, batch, one, repeats):
    """batch: k frames in one call and in k calls; one: the same blocks as one frame through the single calls"""
    row = alternate(torch, {"encode_batch": batch.encode_batch, "encode_singles": batch.encode_singles,
                            "encode_one_frame": one.encode_singles}, repeats)
    torch.cuda.synchronize()
    assert batch.status[0].cpu().tolist() == batch.status[1].cpu().tolist() == [0] * batch.k
    assert torch.equal(batch.frame_bytes[0], batch.frame_bytes[1])
    for f, n in enumerate(batch.frame_bytes[0].cpu().tolist()):
        a = batch.frame_at[f]
        assert torch.equal(batch.frames[0][a:a + n], batch.frames[1][a:a + n]), f
    batch.prepare_decode()
    one.encode_batch()
    torch.cuda.synchronize()
    one.prepare_decode()
    row.update(alternate(torch, {"decode_batch": batch.decode_batch, "decode_singles": batch.decode_singles,
                                 "decode_one_frame": one.decode_singles}, repeats))
    torch.cuda.synchronize()
    assert not batch.err[0].cpu().numpy().any() and not batch.err[1].cpu().numpy().any()
    assert torch.equal(batch.out[0], batch.d_in) and torch.equal(batch.out[1], batch.d_in)
    assert torch.equal(one.out[1], one.d_in)
    for what in ("encode", "decode"):
        b, s, o = (row[f"{what}_{side}"]["median_ms"] for side in ("batch", "singles", "one_frame"))
        row[f"{what}_singles_over_batch"] = round(s / b, 2)
        row[f"{what}_batch_over_one_frame"] = round(b / o, 3)
    row["frames"], row["blocks_per_frame"], row["block_bytes"] = batch.k, batch.blocks, 1 << batch.bits
    row["frame_bytes_total"] = int(batch.frame_bytes[0].sum().item())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--trace", type=int, default=0, metavar="K")
    ap.add_argument("--trace-one", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--layout-probe", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    if a.trace > 0 or a.trace_one:
        if a.small:                                          # (c)'s shapes: frames of one 4 KB block
            s = Shape(1, max(a.trace, 1024), 12) if a.trace_one else Shape(a.trace, 1, 12)
        else:
            s = Shape(1, 256, 18) if a.trace_one else Shape(a.trace, 4, 18)
        torch.cuda.synchronize()
        if a.trace_one:
            s.encode_singles()
            torch.cuda.synchronize()
            for pair in (s.frames, s.frame_bytes, s.status):  # the decode reads side 0
                pair[0].copy_(pair[1])
            s.prepare_decode()
            s.decode_singles()
        else:
            s.encode_batch()
            torch.cuda.synchronize()
            s.prepare_decode()
            s.decode_batch()
        torch.cuda.synchronize()
        assert torch.equal(s.out[1 if a.trace_one else 0], s.d_in)
        print(json.dumps({"ok": True, "traced_frames": 1 if a.trace_one else a.trace, "single_calls": a.trace_one}))
        return
    if a.layout_probe:
        rows = {}
        for blocks in (1, 2, 3, 4, 7):
            batch, one = Shape(1024, blocks, 12), Shape(1, 1024 * blocks, 12)
            for s in (batch, one):
                s.encode_batch()
                torch.cuda.synchronize()
                s.prepare_decode()
            row = alternate(torch, {"decode_batch": batch.decode_batch, "decode_one_frame": one.decode_singles}, a.repeats)
            torch.cuda.synchronize()
            assert torch.equal(batch.out[0], batch.d_in) and torch.equal(one.out[1], one.d_in)
            row["decode_batch_over_one_frame"] = round(row["decode_batch"]["median_ms"] / row["decode_one_frame"]["median_ms"], 3)
            rows[f"{blocks}_blocks_per_frame"] = row
            print(blocks, json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump({"frames": 1024, "block_bytes": 4096, "repeats": a.repeats, "rows": rows}, f, indent=1)
        print(json.dumps({"ok": True}))
        return
    result = {"repeats": a.repeats, "win_bits": WIN_BITS}
    result["a_b_64_frames_of_1MiB"] = compare(torch, Shape(64, 4, 18), Shape(1, 256, 18), a.repeats)
    print(json.dumps(result["a_b_64_frames_of_1MiB"]), flush=True)
    result["c_1024_frames_of_4KB"] = compare(torch, Shape(1024, 1, 12), Shape(1, 1024, 12), a.repeats)
    print(json.dumps(result["c_1024_frames_of_4KB"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main()
