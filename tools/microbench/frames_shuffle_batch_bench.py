"""What byte-shuffled (version 4) frames in the batched frame calls cost and buy, in one GPU visit (DESIGN.md section 10,
"Batches with shuffled frames").  f32 sine content, window 2^15, through the C ABI on torch's current stream.

  a  64 frames of 1 MiB (four 256 KB blocks each), element size 4: sqz_hip_frames_encode_shuf against 64
     sqz_hip_frame_encode_shuf calls on one stream, and sqz_hip_frames_decode_shuf against 64 sqz_hip_frame_decode_shuf
     calls
  b  the filter's cost inside a batch: the same batch against sqz_hip_frames_encode / _decode of the contents shuffled
     beforehand, as version-1 frames, in the same run
  c  the kernel for ranges of mixed element size against what it replaces: 1 GiB as 4096 ranges of 256 KB, element
     sizes cycling 0, 2, 4, 8, both directions -- one sqz_hip_shuffle_ranges launch against three masked launches of the
     kernel of one element size and a masked copy, and against a plain device-to-device copy

The sides of every comparison leave the same bytes (asserted), alternate `--repeats` times after a warm-up of each,
and every figure is a HIP event pair on the launch stream: median and spread (max - min).

  --trace     one batched encode and one batched decode of (a)'s shape and nothing else that launches a kernel of the
              library (the tool's own tensors aside), for `rocprofv3 --kernel-trace --stats -- python ... --trace`
  --trace-single   one sqz_hip_frame_encode_shuf and one sqz_hip_frame_decode_shuf call of ONE such frame, for the same
              kind of run: what a call per frame spends its time on
  --ranges-mib N   (c) over N MiB instead of 1024

    python tools/microbench/frames_shuffle_batch_bench.py [--out profiles/frames_shuffle_batch_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frames_batch_bench import alternate, stats  # noqa: E402,F401

WIN_BITS, BITS, BLOCKS, ELEM = 15, 18, 4, 4
ITEM = [("frame_at", "<u8"), ("avail", "<u8"), ("content_bytes", "<u8"), ("out_at", "<u8"), ("n_blocks", "<u4"),
        ("zero", "<u4")]


def sine(torch, nbytes, jitter=False, device="cuda"):
    """sin(i / 50) as little-endian f32, i = 0 .. nbytes / 4, as bytes on the device.  jitter: every value scaled by
    1 + h(i) / 2^20 with a 10-bit hash h -- the stand-in when the block encoder refuses blocks of the plain sine shuffled
    (E2BIG from the emit kernel's tree guard: DESIGN.md, "A limit of the existing encoder")"""
    i = torch.arange(nbytes // 4, dtype=torch.float64, device=device)
    v = torch.sin(i / 50)
    if jitter:
        h = ((torch.arange(nbytes // 4, dtype=torch.int64, device=device) * 2654435761) >> 7) & 1023
        v = v * (1 + h.to(torch.float64) / (1 << 20))
    return v.to(torch.float32).view(torch.uint8)


class Batch:
    """k frames of BLOCKS blocks of 2^BITS bytes of f32 sine, and what every side of (a) and (b) needs on the device"""

    def __init__(self, k, jitter=False):
        import numpy as np
        import torch
        from sqz_amd import _native as N, frame as F
        self.torch, self.L, self.F, self.k, self.np = torch, N.lib(), F, k, np
        L, p = self.L, F._ptr
        self.size = BLOCKS << BITS
        self.d_in = sine(torch, k * self.size, jitter)
        self.sizes = F._pinned(np.full(k, self.size, np.uint64))
        self.elems = F._pinned(np.full(k, ELEM, np.uint32))
        self.total, self.frame_at = F.frames_bound([self.size] * k, BITS, shuffle=ELEM)
        self.total1, self.frame_at1 = F.frames_bound([self.size] * k, BITS)
        self.room = self.frame_at[1] if k > 1 else self.total
        z32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
        sides = ("batch", "singles", "plain")
        self.frames = {s: torch.zeros(self.total + 16, dtype=torch.uint8, device="cuda") for s in sides}
        self.frame_bytes = {s: torch.zeros(k, dtype=torch.int64, device="cuda") for s in sides}
        self.status = {s: z32(k) for s in sides}
        self.err = {s: z32(k * BLOCKS) for s in sides}
        self.out = {s: torch.zeros(k * self.size, dtype=torch.uint8, device="cuda") for s in sides}
        need = max(int(L.sqz_hip_frames_encode_scratch_bytes_shuf(p(self.sizes), p(self.elems), k, BITS, 0)),
                   int(L.sqz_hip_frame_scratch_bytes_shuf(self.size, BITS, 1, 4)))
        self.scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        # (b): the contents shuffled beforehand, block by block, as a version-4 frame's encoder sees them
        off = torch.arange(k * BLOCKS + 1, dtype=torch.int64, device="cuda") << BITS
        self.d_shuffled = F.shuffle_blocks(self.d_in, off, ELEM)
        torch.cuda.synchronize()

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def check(self, rc):
        assert rc == 0, rc

    def encode_batch(self):
        p = self.F._ptr
        self.check(self.L.sqz_hip_frames_encode_shuf(
            p(self.d_in), p(self.sizes), p(self.elems), self.k, WIN_BITS, BITS, 0, 0, p(self.frames["batch"]), self.total,
            p(self.frame_bytes["batch"]), p(self.status["batch"]), p(self.err["batch"]), p(self.scratch),
            self.scratch.numel(), self.stream()))

    def encode_singles(self):
        s = self.stream()
        for f in range(self.k):
            self.check(self.L.sqz_hip_frame_encode_shuf(
                self.d_in.data_ptr() + f * self.size, self.size, WIN_BITS, BITS, 4, 0, ELEM,
                self.frames["singles"].data_ptr() + self.frame_at[f], self.room,
                self.frame_bytes["singles"].data_ptr() + 8 * f, self.status["singles"].data_ptr() + 4 * f,
                self.err["singles"].data_ptr() + 4 * f * BLOCKS, self.scratch.data_ptr(), self.scratch.numel(), s))

    def encode_plain(self):
        p = self.F._ptr
        self.check(self.L.sqz_hip_frames_encode(
            p(self.d_shuffled), p(self.sizes), self.k, WIN_BITS, BITS, 0, 0, p(self.frames["plain"]), self.total1,
            p(self.frame_bytes["plain"]), p(self.status["plain"]), p(self.err["plain"]), p(self.scratch),
            self.scratch.numel(), self.stream()))

    def table(self, side, frame_at, elem):
        sizes = self.frame_bytes[side].cpu().tolist()
        assert self.status[side].cpu().tolist() == [0] * self.k, self.status[side].cpu().tolist()
        items = self.np.zeros(self.k, self.np.dtype(ITEM))
        for f in range(self.k):
            items[f] = (frame_at[f], sizes[f], self.size, f * self.size, BLOCKS, elem)
        return sizes, self.F._pinned(items)

    def prepare_decode(self, plain=True):
        """after the encodes and a synchronise: the tables of the decodes and their scratch"""
        L, p = self.L, self.F._ptr
        self.sizes_host, self.items = self.table("batch", self.frame_at, ELEM)
        _, self.items1 = self.table("plain", self.frame_at1, 0) if plain else (None, self.items)
        need = max(int(L.sqz_hip_frames_decode_scratch_bytes_shuf(p(self.items), self.k)),
                   int(L.sqz_hip_frames_decode_scratch_bytes(p(self.items1), self.k)),
                   int(L.sqz_hip_frame_scratch_bytes_shuf(self.size, BITS, 0, 4)))
        assert need > 0
        self.dec_scratch = self.torch.empty(need, dtype=self.torch.uint8, device="cuda")

    def decode_batch(self):
        p = self.F._ptr
        self.check(self.L.sqz_hip_frames_decode_shuf(
            p(self.frames["batch"]), p(self.items), self.k, p(self.out["batch"]), p(self.err["batch"]),
            p(self.status["batch"]), p(self.dec_scratch), self.dec_scratch.numel(), self.stream()))

    def decode_singles(self):
        s = self.stream()
        for f in range(self.k):
            self.check(self.L.sqz_hip_frame_decode_shuf(
                self.frames["batch"].data_ptr() + self.frame_at[f], self.sizes_host[f], BLOCKS, self.size, ELEM,
                self.out["singles"].data_ptr() + f * self.size, self.err["singles"].data_ptr() + 4 * f * BLOCKS,
                self.status["singles"].data_ptr() + 4 * f, self.dec_scratch.data_ptr(), self.dec_scratch.numel(), s))

    def decode_plain(self):
        p = self.F._ptr
        self.check(self.L.sqz_hip_frames_decode(
            p(self.frames["plain"]), p(self.items1), self.k, p(self.out["plain"]), p(self.err["plain"]),
            p(self.status["plain"]), p(self.dec_scratch), self.dec_scratch.numel(), self.stream()))


def frames_rows(torch, b, repeats):
    row = alternate(torch, {"encode_batch": b.encode_batch, "encode_singles": b.encode_singles,
                            "encode_plain_batch_of_shuffled_contents": b.encode_plain}, repeats)
    torch.cuda.synchronize()
    assert b.status["batch"].cpu().tolist() == b.status["singles"].cpu().tolist() == [0] * b.k
    assert torch.equal(b.frame_bytes["batch"], b.frame_bytes["singles"])
    for f, n in enumerate(b.frame_bytes["batch"].cpu().tolist()):
        a = b.frame_at[f]
        assert torch.equal(b.frames["batch"][a:a + n], b.frames["singles"][a:a + n]), f
    # the version-1 frames of the shuffled contents carry the same payload, 8 bytes of record less in front of it
    assert torch.equal(b.frame_bytes["batch"] - b.frame_bytes["plain"],
                       torch.full_like(b.frame_bytes["batch"], 16 if BLOCKS % 2 == 0 else 0))
    b.prepare_decode()
    row.update(alternate(torch, {"decode_batch": b.decode_batch, "decode_singles": b.decode_singles,
                                 "decode_plain_batch_of_shuffled_contents": b.decode_plain}, repeats))
    torch.cuda.synchronize()
    for side in ("batch", "singles", "plain"):
        assert not b.err[side].cpu().numpy().any() and not b.status[side].cpu().numpy().any(), side
    assert torch.equal(b.out["batch"], b.d_in) and torch.equal(b.out["singles"], b.d_in)
    assert torch.equal(b.out["plain"], b.d_shuffled)
    for what in ("encode", "decode"):
        bt, s, pl = (row[f"{what}_{side}"]["median_ms"] for side in ("batch", "singles",
                                                                    "plain_batch_of_shuffled_contents"))
        row[f"{what}_singles_over_batch"] = round(s / bt, 2)
        row[f"{what}_batch_over_plain_batch"] = round(bt / pl, 3)
    row["frames"], row["blocks_per_frame"], row["block_bytes"], row["elem_bytes"] = b.k, BLOCKS, 1 << BITS, ELEM
    row["frame_bytes_total"] = int(b.frame_bytes["batch"].sum().item())
    row["content_bytes_total"] = b.k * b.size
    return row


def ranges_rows(torch, mib, repeats):
    from sqz_amd import _native as N, frame as F
    L, p = N.lib(), F._ptr
    n = max(mib * 4, 4)                                      # ranges of 256 KB
    total = n << BITS
    cycle = (0, 2, 4, 8)
    d_src = sine(torch, total)
    d_one = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_many = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_copy = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_off = torch.arange(n + 1, dtype=torch.int64, device="cuda") << BITS
    elems = torch.tensor([cycle[j % 4] for j in range(n)], dtype=torch.int32, device="cuda")
    skip_for = {e: (elems != e).to(torch.int32) for e in (2, 4, 8)}      # the masked launches: the others are left alone
    take_0 = (elems == 0).to(torch.int32)                                # the masked copy: its mask says which to take
    torch.cuda.synchronize()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = {}
    for inverse in (0, 1):
        src = d_src if inverse == 0 else d_one.clone()       # inverse: back from what the forward pass left

        def one_launch():
            assert L.sqz_hip_shuffle_ranges(p(src), p(d_off), p(elems), n, inverse, p(d_one if inverse == 0 else d_many),
                                            None, stream()) == 0

        def masked_launches():
            dst = d_many if inverse == 0 else d_copy
            for e in (2, 4, 8):
                assert L.sqz_hip_shuffle_blocks_masked(p(src), p(d_off), n, e, inverse, p(dst), p(skip_for[e]),
                                                       stream()) == 0
            assert L.sqz_hip_shuffle_blocks_masked(p(src), p(d_off), n, 0, inverse, p(dst), p(take_0), stream()) == 0

        scratch = torch.empty_like(d_src)

        def plain_copy():
            scratch.copy_(src)

        row = alternate(torch, {"one_launch": one_launch, "masked_launches": masked_launches,
                                "device_to_device_copy": plain_copy}, repeats)
        torch.cuda.synchronize()
        if inverse == 0:
            assert torch.equal(d_one, d_many) and not torch.equal(d_one, d_src)
        else:
            assert torch.equal(d_many, d_copy) and torch.equal(d_many, d_src)
        one, many, cp = (row[s]["median_ms"] for s in ("one_launch", "masked_launches", "device_to_device_copy"))
        row["masked_over_one_launch"] = round(many / one, 3)
        row["one_launch_over_copy"] = round(one / cp, 3)
        row["one_launch_GBps_read_plus_written"] = round(2 * total / one / 1e6, 1)
        row["copy_GBps_read_plus_written"] = round(2 * total / cp / 1e6, 1)
        rows["inverse" if inverse else "forward"] = row
    rows["ranges"], rows["range_bytes"], rows["elem_cycle"] = n, 1 << BITS, list(cycle)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--ranges-mib", type=int, default=1024)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-single", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    if a.trace or a.trace_single:
        b = Batch(1 if a.trace_single else a.frames)
        side = "singles" if a.trace_single else "batch"
        (b.encode_singles if a.trace_single else b.encode_batch)()
        torch.cuda.synchronize()
        if a.trace_single:                                   # the decode reads side "batch"
            for pair in (b.frames, b.frame_bytes, b.status):
                pair["batch"].copy_(pair["singles"])
        b.prepare_decode(plain=False)
        (b.decode_singles if a.trace_single else b.decode_batch)()
        torch.cuda.synchronize()
        assert torch.equal(b.out[side], b.d_in) and not b.err[side].cpu().numpy().any()
        print(json.dumps({"ok": True, "traced_frames": b.k, "single_calls": a.trace_single}))
        return
    result = {"repeats": a.repeats, "win_bits": WIN_BITS, "content": "f32 sine"}
    b = Batch(a.frames)
    b.encode_batch()
    torch.cuda.synchronize()
    refused = [s for s in b.status["batch"].cpu().tolist() if s != 0]
    if refused:                                              # said, not hidden: the figures below are the stand-in's
        result["f32_sine_frames_refused"] = {"frames": len(refused), "errno": refused[0]}
        result["content"] = "f32 sine, every value scaled by 1 + h(i) / 2^20"
        b = Batch(a.frames, jitter=True)
    result["a_b_frames_of_1MiB_f32_sine"] = frames_rows(torch, b, a.repeats)
    print(json.dumps(result["a_b_frames_of_1MiB_f32_sine"]), flush=True)
    result["c_ranges_of_mixed_element_size"] = ranges_rows(torch, a.ranges_mib, a.repeats)
    print(json.dumps(result["c_ranges_of_mixed_element_size"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main()
