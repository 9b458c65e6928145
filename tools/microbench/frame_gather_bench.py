"""What a gather of many ranges from a resident frame buys, in one GPU visit.

The workload is dict_bench.py's: 16,384 blocks of 4 KB cut from confucius.txt behind its first 32,767 bytes, which
are the dictionary, as one version-3 frame (store=True), and the same content as a version-1 frame.  For R = 1, 64,
4,096 and 65,536 uniformly random ranges of 256 bytes, and R = 4,096 ranges of 16 KB:

  a  one gather_frame call (offsets and lengths device tensors)
  b  R read_frame calls, one range each, the way there was (up to R = 4,096: 65,536 calls are not measured)
  c  decode_frame of the whole frame, then a torch gather of the ranges out of the decoded content

Sides alternate `--repeats` times after a warm-up of each; every figure is a HIP event pair on the launch stream;
median and spread (max - min).  For (a) the per-kernel times of sqz_hip_get_timing are recorded in a run of their
own, and the two copy kernels are timed against each other on the same ranges (max_length just under and just over
the switch, which changes the kernel and nothing else).

    python tools/microbench/frame_gather_bench.py [--out profiles/frame_gather_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WIN_BITS, BLOCK_BITS = 15, 12
SWITCH = 4096                                   # sqzk_gather_copy_max (sqz_amd/csrc/abi.hip)


def stats(xs):
    return {"ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
            "spread_ms": round(max(xs) - min(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--most-reads", type=int, default=4096, help="(b) is measured up to this many ranges")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from dict_bench import bench_blocks
    from sqz_amd import _native as N, frame as F
    L = N.lib()
    n = a.blocks
    dct, flat, bb = bench_blocks(n)
    assert bb == 1 << BLOCK_BITS
    total = n * bb
    d_in = torch.from_numpy(flat.copy()).cuda()
    d_dict = torch.from_numpy(np.frombuffer(dct, np.uint8).copy()).cuda()
    back = torch.empty(total, dtype=torch.uint8, device="cuda")

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), res

    result = {"blocks": n, "block_bytes": bb, "repeats": a.repeats, "frames": {}}
    for version in (3, 1):
        dictionary = d_dict if version == 3 else None
        enc = F.FrameEncoder(total, WIN_BITS, BLOCK_BITS, store=version == 3, dictionary=dictionary)
        enc.encode(d_in)
        host = enc.result()
        info = F.frame_info(host)
        assert info["version"] == version
        frame = enc.frame[:len(host)]
        rows = {}
        for count, length in ((1, 256), (64, 256), (4096, 256), (65536, 256), (4096, 16384)):
            g = torch.Generator(device="cuda").manual_seed(count + length)
            offsets = torch.randint(0, total - length, (count,), generator=g, device="cuda", dtype=torch.int64)
            lengths = torch.full((count,), length, dtype=torch.int64, device="cuda")
            d_out = torch.empty(count * length, dtype=torch.uint8, device="cuda")
            h_off = offsets.cpu().tolist()
            index = (offsets[:, None] + torch.arange(length, device="cuda")[None, :]).reshape(-1)

            def side_a(cap=length):
                return F.gather_frame(frame, offsets, lengths, max_length=cap, d_out=d_out, info=info, dictionary=dictionary)

            def side_b():
                for r in range(count):
                    F.read_frame(frame, h_off[r], length, d_out=d_out[r * length:], info=info, dictionary=dictionary)

            def side_c():
                F.decode_frame(frame, back, info=info, dictionary=dictionary)
                return back[index]

            sides = {"a_gather": side_a, "c_decode_all_then_gather": side_c}
            if count <= a.most_reads:
                sides["b_one_read_each"] = side_b
            want = back.new_empty(0)
            for name, fn in sides.items():                  # warm-up of every side, and all three agree
                fn()
            torch.cuda.synchronize()
            want = side_c()
            out, out_off, rerr, dec, st = side_a()
            torch.cuda.synchronize()
            assert int(st.item()) == 0 and int(rerr.abs().sum()) == 0 and torch.equal(out[:count * length], want)
            times = {k: [] for k in sides}
            for _ in range(a.repeats):
                for name, fn in sides.items():
                    times[name].append(timed(fn)[0])
            row = {k: stats(v) for k, v in times.items()}
            row["blocks_decoded"] = int(dec.item())
            # (a)'s kernels, in a run of their own
            L.sqz_hip_set_timing(1)
            side_a()
            torch.cuda.synchronize()
            t = N.Timing()
            L.sqz_hip_get_timing(C.byref(t), 1)
            L.sqz_hip_set_timing(0)
            row["a_kernels_ms"] = {f: [round(float(x), 4) for x in getattr(t, f)] if hasattr(getattr(t, f), "__len__")
                                   else round(float(getattr(t, f)), 4) for f, _ in N.Timing._fields_}
            # the two copy kernels on the same work list: max_length on either side of the switch
            if length <= SWITCH:
                small, wide = [], []
                for _ in range(a.repeats):
                    small.append(timed(lambda: side_a(SWITCH))[0])
                    wide.append(timed(lambda: side_a(SWITCH + 1))[0])
                row["whole_call_gather_copy"] = stats(small)
                row["whole_call_range_copy"] = stats(wide)
            rows[f"R{count}_x{length}"] = row
            print(version, count, length, {k: v["median_ms"] for k, v in row.items() if isinstance(v, dict) and "median_ms" in v}, flush=True)
        result["frames"][f"version_{version}"] = rows
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main()
