"""What SQZF version 2 (stored blocks) costs and buys, measured against the PARENT commit's tree in one GPU visit.

  1  nothing existing got slower: `python bench.py --steps 20 --warmup 5` and the decode figure of
     `python bench.py --full`, the parent's tree and this tree alternating (child processes: bench.py is one);
  2  version 2 costs nothing where nothing is stored: the bench batch (4096 x 256 KB Zipf) as a version-1 frame by
     the parent's library (the baseline), as a version-1 and as a version-2 frame by this one, encode and decode;
  3  what it buys: 1024 blocks of 256 KB with every fourth one noise, and 256 MiB of noise -- the parent's decode
     of the version-1 frame against this tree's decode of the version-2 frame, the sizes of both frames, and
     the copy kernel's rate against the 8 TB/s of the HBM.

2 and 3 run in ONE process that has both libraries loaded (ctypes, the C ABI of include/sqz/sqz.h); the sides
alternate `--repeats` times after a warm-up of each; every figure is a HIP event pair on the launch stream; median
and spread (max - min) are reported (the copy kernel's own time: median of `--repeats` launches, timing slot 11).  Asserted: only the direction of 3 (version-2 decode faster, version-2
frame not larger than content + index + 54 bytes) and that every decode gives the content back.

    python tools/microbench/frame_store_bench.py --parent-tree DIR [--repeats 5] [--out profiles/frame_store_bench.json]

DIR: a checkout of the parent commit with its library built (python -m sqz_amd.build)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X
STORED = 1


def stats(xs):
    return {"ms": [round(x, 3) for x in xs], "median_ms": round(statistics.median(xs), 3),
            "spread_ms": round(max(xs) - min(xs), 3)}


class Lib:
    """one libsqz_amd.so through ctypes: the device flavour of the frame calls over torch tensors"""

    def __init__(self, path, has_ex):
        import torch
        self.torch = torch
        self.h = C.CDLL(path)
        self.has_ex = has_ex
        self.h.sqz_frame_bound.restype = C.c_uint64
        self.h.sqz_frame_bound.argtypes = [C.c_uint64, C.c_uint32]
        self.h.sqz_hip_frame_scratch_bytes.restype = C.c_uint64
        self.h.sqz_hip_frame_scratch_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_int]
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        self.h.sqz_hip_frame_encode.argtypes = [vp, u64, u32, u32, vp, u64, vp, vp, vp, vp, u64, vp]
        self.h.sqz_hip_frame_decode.argtypes = [vp, u64, u32, u64, vp, vp, vp, vp, u64, vp]
        if has_ex:
            self.h.sqz_frame_bound_ex.restype = C.c_uint64
            self.h.sqz_frame_bound_ex.argtypes = [u64, u32, u32]
            self.h.sqz_hip_frame_scratch_bytes_ex.restype = C.c_uint64
            self.h.sqz_hip_frame_scratch_bytes_ex.argtypes = [u64, u32, C.c_int, u32]
            self.h.sqz_hip_frame_encode_ex.argtypes = [vp, u64, u32, u32, u32, vp, u64, vp, vp, vp, vp, u64, vp]
        self.h.sqz_hip_set_timing.argtypes = [C.c_int]
        self.scratch = None

    def _scratch(self, need):
        if self.scratch is None or self.scratch.numel() < need:
            self.scratch = self.torch.empty(need, dtype=self.torch.uint8, device="cuda")
        return self.scratch

    def encoder(self, content, wb, bits, flags):
        """-> fn() that enqueues one encode of d_in and returns (frame, frame_bytes, status, err)"""
        t = self.torch
        cap = self.h.sqz_frame_bound_ex(content, bits, flags) if flags else self.h.sqz_frame_bound(content, bits)
        need = self.h.sqz_hip_frame_scratch_bytes_ex(content, bits, 1, flags) if flags else \
            self.h.sqz_hip_frame_scratch_bytes(content, bits, 1)
        n = (content + (1 << bits) - 1) >> bits
        frame = t.empty(cap, dtype=t.uint8, device="cuda")
        fb = t.zeros(1, dtype=t.int64, device="cuda")
        st = t.zeros(1, dtype=t.int32, device="cuda")
        err = t.zeros(max(n, 1), dtype=t.int32, device="cuda")
        scratch = t.empty(need, dtype=t.uint8, device="cuda")
        p = lambda x: C.c_void_p(x.data_ptr())

        def run(d_in):
            stream = C.c_void_p(t.cuda.current_stream().cuda_stream)
            if flags:
                rc = self.h.sqz_hip_frame_encode_ex(p(d_in), content, wb, bits, flags, p(frame), cap, p(fb), p(st), p(err),
                                                    p(scratch), need, stream)
            else:
                rc = self.h.sqz_hip_frame_encode(p(d_in), content, wb, bits, p(frame), cap, p(fb), p(st), p(err),
                                                 p(scratch), need, stream)
            assert rc == 0, rc
            return frame, fb, st, err
        return run

    def decode(self, d_frame, n, content, bits, d_out, err, st):
        t = self.torch
        need = self.h.sqz_hip_frame_scratch_bytes(content, bits, 0)
        scratch = self._scratch(need)
        p = lambda x: C.c_void_p(x.data_ptr())
        rc = self.h.sqz_hip_frame_decode(p(d_frame), d_frame.numel(), n, content, p(d_out), p(err), p(st), p(scratch),
                                         scratch.numel(), C.c_void_p(t.cuda.current_stream().cuda_stream))
        assert rc == 0, rc


def bench_py(tree, extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--cpu-blocks", "0"] + extra
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-repeats", type=int, default=5)
    ap.add_argument("--full-repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--commit", default=os.environ.get("SQZ_COMMIT", "unknown"),
                    help="the parent commit's id (recorded, not checked)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"what": "SQZF version 2 (stored blocks) against the parent commit's tree, one GPU visit", "parent_commit": a.commit,
           "repeats": a.repeats}

    def flush():
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    # ---- 1. bench.py, child processes, alternating ----
    enc = {"parent": [], "this": []}
    for _ in range(a.bench_repeats):
        for side, tree in (("parent", a.parent_tree), ("this", ROOT)):
            enc[side].append(bench_py(tree, ["--steps", "20", "--warmup", "5"])["value"])
            print("bench.py encode", side, enc[side][-1], "MB/s", flush=True)
    dec = {"parent": [], "this": []}
    for _ in range(a.full_repeats):
        for side, tree in (("parent", a.parent_tree), ("this", ROOT)):
            dec[side].append(bench_py(tree, ["--full", "--steps", "3", "--warmup", "1"])["decode_MBps"])
            print("bench.py --full decode", side, dec[side][-1], "MB/s", flush=True)
    res["bench_py"] = {
        "encode_command": "python bench.py --gpus 1 --cpu-blocks 0 --steps 20 --warmup 5",
        "decode_command": "python bench.py --gpus 1 --cpu-blocks 0 --full --steps 3 --warmup 1 (decode_MBps)",
        "parent_encode_MBps": enc["parent"], "this_encode_MBps": enc["this"],
        "parent_decode_MBps": dec["parent"], "this_decode_MBps": dec["this"],
        "parent_encode_median": statistics.median(enc["parent"]), "this_encode_median": statistics.median(enc["this"]),
        "parent_encode_spread": round(max(enc["parent"]) - min(enc["parent"]), 3),
        "parent_decode_median": statistics.median(dec["parent"]), "this_decode_median": statistics.median(dec["this"]),
        "parent_decode_spread": round(max(dec["parent"]) - min(dec["parent"]), 3)}
    print(json.dumps(res["bench_py"]), flush=True)
    flush()

    # ---- 2 and 3: one process, both libraries ----
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "frame_store_bench.py needs a GPU: there is nothing to measure without one"
    import sqz_amd
    from sqz_amd import batch, frame as F, _native
    res["device"] = sqz_amd.device_info()["name"]
    this = Lib(_native.LIB_PATH, True)
    parent = Lib(os.path.join(a.parent_tree, "sqz_amd", "lib", "libsqz_amd.so"), False)
    bits, wb = 18, 15
    bb = 1 << bits

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), r

    def frame_of(run, d_in):
        frame, fb, st, err = run(d_in)
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and int(err.abs().sum()) == 0
        return frame[:int(fb.item())].clone()

    def copy_kernel(fn):
        """slot 11 of this tree's library around one call: (median ms of `--repeats` calls, launches per call)"""
        batch.set_timing(True)
        ms, launches = [], 0
        for _ in range(a.repeats):
            batch.get_timing(reset=True)
            fn()
            torch.cuda.synchronize()
            t = batch.get_timing(reset=True).get("range_copy_kernel", (0.0, 0))
            ms.append(t[0])
            launches = t[1]
        batch.set_timing(False)
        return statistics.median(ms), launches

    def section(name, d_in, n):
        content = n * bb
        sides = {"parent_v1": parent.encoder(content, wb, bits, 0), "this_v1": this.encoder(content, wb, bits, 0),
                 "this_v2": this.encoder(content, wb, bits, STORED)}
        for run in sides.values():
            run(d_in)
        torch.cuda.synchronize()
        et = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, run in sides.items():
                ms, (frame, fb, st, err) = timed(lambda: run(d_in))
                assert int(st.item()) == 0 and int(err.abs().sum()) == 0
                et[k].append(ms)
        frames = {k: frame_of(run, d_in) for k, run in sides.items()}
        assert torch.equal(frames["parent_v1"], frames["this_v1"]), "the version-1 frame changed"
        enc_copy = copy_kernel(lambda: sides["this_v2"](d_in))
        del sides
        torch.cuda.empty_cache()
        blocks = F.frame_blocks(frames["this_v2"][:32 + 8 * n + 8].cpu().numpy().tobytes()) if n <= 4096 else []
        n_stored = sum(b["stored"] for b in blocks)
        d_out = torch.empty_like(d_in)
        err = torch.zeros(n, dtype=torch.int32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        decs = {"parent_v1": (parent, frames["parent_v1"]), "this_v1": (this, frames["this_v1"]),
                "this_v2": (this, frames["this_v2"])}
        for lib, fr in decs.values():
            lib.decode(fr, n, content, bits, d_out, err, st)
        torch.cuda.synchronize()
        dt = {k: [] for k in decs}
        for _ in range(a.repeats):
            for k, (lib, fr) in decs.items():
                d_out.zero_()
                ms, _ = timed(lambda: lib.decode(fr, n, content, bits, d_out, err, st))
                assert int(st.item()) == 0 and int(err.abs().sum()) == 0 and torch.equal(d_out, d_in), (name, k)
                dt[k].append(ms)
        dec_copy = copy_kernel(lambda: this.decode(frames["this_v2"], n, content, bits, d_out, err, st))
        dec_copy_v1 = copy_kernel(lambda: this.decode(frames["this_v1"], n, content, bits, d_out, err, st))
        moved = n_stored * bb
        out = {"blocks": n, "content_bytes": content, "stored_blocks": n_stored,
               "frame_bytes_v1": frames["this_v1"].numel(), "frame_bytes_v2": frames["this_v2"].numel(),
               "encode": {k: stats(v) for k, v in et.items()}, "decode": {k: stats(v) for k, v in dt.items()},
               "copy_kernel_encode_ms": round(enc_copy[0], 4), "copy_kernel_decode_ms": round(dec_copy[0], 4),
               "copy_kernel_decode_ms_on_v1_frame": round(dec_copy_v1[0], 4)}
        if moved and dec_copy[0] > 0:      # read + write of every stored byte
            out["copy_kernel_decode_GBps"] = round(2 * moved / (dec_copy[0] * 1e-3) / 1e9, 1)
            out["copy_kernel_encode_GBps"] = round(2 * moved / (enc_copy[0] * 1e-3) / 1e9, 1)
            out["copy_kernel_decode_share_of_hbm_peak_percent"] = round(100 * 2 * moved / (dec_copy[0] * 1e-3) / HBM_PEAK, 1)
        res[name] = out
        print(name, json.dumps(out), flush=True)
        flush()
        return out

    # 2. the bench batch: nothing stored
    d = batch.zipf_blocks(a.blocks, bb)
    r = section("bench_batch", d, a.blocks)
    assert r["stored_blocks"] == 0
    base = r["decode"]["parent_v1"]
    r["judgement"] = {"margin_ms": "the baseline's spread plus the copy kernel's own time",
                      "encode_v2_minus_parent_ms": round(r["encode"]["this_v2"]["median_ms"] - r["encode"]["parent_v1"]["median_ms"], 3),
                      "encode_margin_ms": round(r["encode"]["parent_v1"]["spread_ms"] + r["copy_kernel_encode_ms"], 3),
                      "decode_v2_minus_parent_ms": round(r["decode"]["this_v2"]["median_ms"] - base["median_ms"], 3),
                      "decode_v1_minus_parent_ms": round(r["decode"]["this_v1"]["median_ms"] - base["median_ms"], 3),
                      "decode_margin_ms": round(base["spread_ms"] + r["copy_kernel_decode_ms"], 3)}
    del d
    torch.cuda.empty_cache()

    # 3. mixed: every fourth block noise; all noise
    n = 1024
    d = batch.zipf_blocks(n, bb)
    g = torch.Generator(device="cuda").manual_seed(41)
    d.view(n, bb)[3::4] = torch.randint(0, 256, (n // 4, bb), dtype=torch.uint8, device="cuda", generator=g)
    r = section("mixed_1024", d, n)
    assert r["stored_blocks"] == n // 4
    d = torch.randint(0, 256, (n * bb,), dtype=torch.uint8, device="cuda", generator=g)
    r2 = section("noise_256MiB", d, n)
    assert r2["stored_blocks"] == n
    for x in (r, r2):
        assert x["decode"]["this_v2"]["median_ms"] < x["decode"]["parent_v1"]["median_ms"], "version-2 decode is not faster"
        assert x["frame_bytes_v2"] <= x["content_bytes"] + 8 * x["blocks"] + 54, "version-2 frame is larger than its bound"
    flush()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
