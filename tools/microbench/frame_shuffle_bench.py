"""What the byte-shuffle filter of SQZF version 4 costs, in one GPU visit.

  a  shuffle_blocks_kernel against a plain device-to-device copy of the same bytes: 1 GiB as 4096 ranges of 256 KB,
     elements of 2, 4 and 8 bytes, forward and inverse.  The kernel reads and writes every byte once, as the copy does.
  b  the encode and the decode step of a version-4 frame against a version-1 frame of the ALREADY SHUFFLED content
     (the same streams): the difference is the filter's cost.  Content: the `f32` sine of the payload table, repeated
     to --frame-mb MB, blocks of 256 KB.
  c  the payload table of README / DESIGN.md once more, from the frames this build writes, next to the CPU model's
     figures (tests/frame_writer_v4.py); a row the encoder refuses is recorded with its errno.

Sides alternate `--repeats` times after a warm-up of each; every figure is a HIP event pair on the launch stream;
median and spread (max - min).

    python tools/microbench/frame_shuffle_bench.py [--out profiles/frame_shuffle_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(xs):
    return {"ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
            "spread_ms": round(max(xs) - min(xs), 4)}


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(torch, sides, repeats):
    """sides: {name: callable}; a warm-up of each, then `repeats` rounds in which they take turns"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    got = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            got[k].append(timed(torch, fn))
    return {k: stats(v) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--range-kb", type=int, default=256)
    ap.add_argument("--frame-mb", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    import sqz_amd
    from sqz_amd import frame as F
    import frame_writer_v4 as W4
    result = {"device": sqz_amd.device_info()["name"], "repeats": a.repeats}

    # ---- a: the kernel against a copy
    size = a.range_kb * 1024
    total = a.ranges * size
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    off = torch.arange(a.ranges + 1, dtype=torch.int64, device="cuda") * size
    rows = {}
    for e in (2, 4, 8):
        for inverse in (False, True):
            row = alternate(torch, {"shuffle": lambda: F.shuffle_blocks(src, off, e, inverse, d_out=dst),
                                    "copy": lambda: dst.copy_(src)}, a.repeats)
            row["bytes"] = total
            row["shuffle_gb_s"] = round(2 * total / row["shuffle"]["median_ms"] / 1e6, 1)    # read + written
            row["copy_gb_s"] = round(2 * total / row["copy"]["median_ms"] / 1e6, 1)
            row["ratio"] = round(row["shuffle"]["median_ms"] / row["copy"]["median_ms"], 3)
            rows[f"e{e}_{'inverse' if inverse else 'forward'}"] = row
            print("a", e, inverse, row["shuffle"]["median_ms"], row["copy"]["median_ms"], row["ratio"], flush=True)
    result["a_kernel_vs_copy"] = rows
    del src, dst

    # ---- b: whole-frame steps
    try:
        whole_frame_steps(a, torch, np, sqz_amd, F, W4, result)
    except sqz_amd.SqzError as err:                          # an encoder's refusal is a finding, and (c) still runs
        result["b_error"] = f"errno {err.errno}: {err}"
        print("b", result["b_error"], flush=True)
    payload_table(sqz_amd, W4, result)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"ok": True}))


def whole_frame_steps(a, torch, np, sqz_amd, F, W4, result):
    bits, e = 18, 4
    ramp = W4.figure_input("f32_sine")[:16388]
    content = (ramp * (a.frame_mb * (1 << 20) // len(ramp) + 1))[:a.frame_mb << 20]
    d_in = torch.from_numpy(np.frombuffer(content, np.uint8).copy()).cuda()
    n = len(content) >> bits
    cuts = torch.arange(n + 1, dtype=torch.int64, device="cuda") << bits
    d_pre = F.shuffle_blocks(d_in, cuts, e)
    enc4 = F.FrameEncoder(len(content), 15, bits, shuffle=e)
    enc1 = F.FrameEncoder(len(content), 15, bits)
    row = alternate(torch, {"v4": lambda: enc4.encode(d_in), "v1_preshuffled": lambda: enc1.encode(d_pre)}, a.repeats)
    f4, f1 = enc4.result(), enc1.result()
    i4, i1 = sqz_amd.frame_info(f4), sqz_amd.frame_info(f1)
    assert i4["payload_bytes"] == i1["payload_bytes"], "the same streams"
    row["content_bytes"], row["payload_bytes"] = len(content), i4["payload_bytes"]
    row["filter_ms"] = round(row["v4"]["median_ms"] - row["v1_preshuffled"]["median_ms"], 4)
    result["b_encode"] = row
    print("b encode", row["v4"]["median_ms"], row["v1_preshuffled"]["median_ms"], flush=True)
    d4, d1 = enc4.frame[:len(f4)], enc1.frame[:len(f1)]
    out4, out1 = torch.empty(len(content), dtype=torch.uint8, device="cuda"), torch.empty(len(content), dtype=torch.uint8, device="cuda")
    row = alternate(torch, {"v4": lambda: F.decode_frame(d4, out4, info=i4),
                            "v1_preshuffled": lambda: F.decode_frame(d1, out1, info=i1)}, a.repeats)
    torch.cuda.synchronize()
    assert torch.equal(out4, d_in) and torch.equal(out1, d_pre)
    row["filter_ms"] = round(row["v4"]["median_ms"] - row["v1_preshuffled"]["median_ms"], 4)
    result["b_decode"] = row
    print("b decode", row["v4"]["median_ms"], row["v1_preshuffled"]["median_ms"], flush=True)



def payload_table(sqz_amd, W4, result):
    table = {}
    for name, eb in W4.FIGURES:
        data = W4.figure_input(name)
        for bb in (12, 13):
            cell = {"model_plain": W4.model_payload(name, 0, bb), "model_shuffled": W4.model_payload(name, eb, bb)}
            for key, kw in (("gpu_plain", {}), ("gpu_shuffled", {"shuffle": eb})):
                try:
                    cell[key] = sqz_amd.frame_info(sqz_amd.compress_frame(data, 15, bb, **kw))["payload_bytes"]
                except sqz_amd.SqzError as err:
                    cell[key] = f"errno {err.errno}"
            cell["equal"] = cell["gpu_plain"] == cell["model_plain"] and cell["gpu_shuffled"] == cell["model_shuffled"]
            table[f"{name}_e{eb}_b{bb}"] = cell
            print("c", name, bb, cell, flush=True)
    result["c_payload_table"] = table


if __name__ == "__main__":
    main()
