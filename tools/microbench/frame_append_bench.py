"""What appending to a resident frame in one call buys, in one GPU visit.

The workload is dict_bench.py's: 16,384 blocks of 4 KB cut from confucius.txt behind its first 32,767 bytes, which
are the dictionary, as one version-3 frame (store=True), and the same content as a version-1 frame -- less its last
3,000 bytes, so that the old content ends in mid-block and an append touches the last block.  For 256 bytes, 64 KiB
and 4 MiB of the same text behind it:

  a  one append_frame call (the data a device tensor)
  b  the way there was: decode_frame of the whole frame, the data copied behind the decoded content,
     FrameEncoder.encode over every block

Both sides leave the same frame (asserted).  Sides alternate `--repeats` times after a warm-up of each; every figure is
a HIP event pair on the launch stream; median and spread (max - min).  For (a) the per-kernel times of
sqz_hip_get_timing are recorded in a run of their own: SQZ_HIP_K_RANGE_COPY holds the touched block's stored copy, the
staging copy of the data and frame_splice_kernel, of which the splice is all but a few microseconds for a large frame,
so its bytes per second (the new payload, read once and written once) are worked out from that slot.

    python tools/microbench/frame_append_bench.py [--out profiles/frame_append_bench.json]
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
K_RANGE_COPY = 11                               # SQZ_HIP_K_RANGE_COPY (include/sqz/sqz.h)
CUT = 3000                                      # bytes left off the last block of the old content


def stats(xs):
    return {"ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
            "spread_ms": round(max(xs) - min(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
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
    old_bytes = n * bb - CUT
    sizes = (256, 64 << 10, 4 << 20)
    most = old_bytes + max(sizes)
    supply = np.resize(flat, max(sizes))                    # the same text again, as the data
    d_old = torch.from_numpy(flat[:old_bytes].copy()).cuda()
    d_supply = torch.from_numpy(supply.copy()).cuda()
    d_dict = torch.from_numpy(np.frombuffer(dct, np.uint8).copy()).cuda()
    back = torch.empty(most, dtype=torch.uint8, device="cuda")

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), res

    result = {"blocks": n, "block_bytes": bb, "old_content_bytes": old_bytes, "repeats": a.repeats, "frames": {}}
    for version in (3, 1):
        dictionary = d_dict if version == 3 else None
        enc = F.FrameEncoder(most, WIN_BITS, BLOCK_BITS, store=version == 3, dictionary=dictionary)
        enc.encode(d_old)
        host = enc.result()
        info = F.frame_info(host)
        assert info["version"] == version and info["content_bytes"] == old_bytes
        frame = enc.frame[:len(host)].clone()
        d_new = torch.empty(F.frame_bound(most, BLOCK_BITS, store=version == 3, dictionary=version == 3), dtype=torch.uint8,
                            device="cuda")
        rows = {}
        for size in sizes:
            data = d_supply[:size]

            def side_a():
                return F.append_frame(frame, data, d_out=d_new, info=info, dictionary=dictionary)

            def side_b():
                F.decode_frame(frame, back, info=info, dictionary=dictionary)
                back[old_bytes:old_bytes + size] = data
                enc.encode(back, old_bytes + size)

            for fn in (side_a, side_b):                     # warm-up of either side, and both leave the same frame
                fn()
            torch.cuda.synchronize()
            out, fb, blocks, st = side_a()
            torch.cuda.synchronize()
            new_bytes = int(fb.item())
            assert int(st.item()) == 0 and int(enc.status.item()) == 0 and new_bytes == int(enc.frame_bytes.item())
            assert torch.equal(out[:new_bytes], enc.frame[:new_bytes])
            times = {"a_append": [], "b_decode_concat_encode": []}
            for _ in range(a.repeats):
                times["a_append"].append(timed(side_a)[0])
                times["b_decode_concat_encode"].append(timed(side_b)[0])
            row = {k: stats(v) for k, v in times.items()}
            row["blocks_encoded"] = int(blocks.item())
            row["frame_bytes"] = new_bytes
            L.sqz_hip_set_timing(1)
            side_a()
            torch.cuda.synchronize()
            t = N.Timing()
            L.sqz_hip_get_timing(C.byref(t), 1)
            L.sqz_hip_set_timing(0)
            row["a_kernels_ms"] = {f: [round(float(x), 4) for x in getattr(t, f)] if hasattr(getattr(t, f), "__len__")
                                   else round(float(getattr(t, f)), 4) for f, _ in N.Timing._fields_}
            copy_ms = float(t.ms[K_RANGE_COPY])
            row["range_copy_slot_ms"] = round(copy_ms, 4)
            payload = new_bytes - F.frame_info(out[:32].cpu().numpy().tobytes())["payload_off"]
            row["splice_gb_per_s_read_plus_write"] = round(2 * payload / copy_ms / 1e6, 1) if copy_ms > 0 else None
            rows[f"A{size}"] = row
            print(version, size, {k: v["median_ms"] for k, v in row.items() if isinstance(v, dict) and "median_ms" in v},
                  row["splice_gb_per_s_read_plus_write"], flush=True)
        result["frames"][f"version_{version}"] = rows
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main()
