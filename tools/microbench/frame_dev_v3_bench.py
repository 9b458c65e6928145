"""What the device-resident version-3 frame and the ranged read from a resident frame cost, in one GPU visit.

The workload is dict_bench.py's: 16,384 blocks of 4 KB cut from confucius.txt behind its first 32,767 bytes, which
are the dictionary; window 2^15, block_bits 12, everything device resident.  Sides alternate `--repeats` times after
a warm-up of each; every device figure is a HIP event pair on the launch stream; median and spread (max - min).

  a  encode: sqz_hip_encode_blocks_dict + sqz_hip_pack_blocks (side A) against FrameEncoder(dictionary=) (side B)
  b  decode: sqz_hip_decode_blocks_dict of the packed streams (A) against decode_frame(dictionary=) (B)
  c  ranged reads: read_frame of one aligned 4 KB block and of 64 KB across 17 blocks from the resident frame (B,
     event pair) against the host read_range(..., dictionary=) of the same ranges on a host copy of the frame (A,
     wall clock: it uploads header, index and the covering streams, decodes, and copies the range back)

    python tools/microbench/frame_dev_v3_bench.py [--out profiles/frame_dev_v3_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WIN_BITS, BLOCK_BITS = 15, 12


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
    import sqz_amd
    from dict_bench import bench_blocks
    from sqz_amd import _native as N, batch, frame as F
    L = N.lib()
    n, window = a.blocks, 1 << WIN_BITS
    dct, flat, bb = bench_blocks(n)
    assert bb == 1 << BLOCK_BITS
    total = n * bb
    d_in = torch.from_numpy(flat.copy()).cuda()
    d_dict = torch.from_numpy(np.frombuffer(dct, np.uint8).copy()).cuda()
    in_off = torch.arange(0, (n + 1) * bb, bb, dtype=torch.int64, device="cuda")
    cap = int(L.sqz_bound(bb))
    slab_off = torch.arange(0, (n + 1) * cap, cap, dtype=torch.int64, device="cuda")
    slabs = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    err = torch.zeros(n, dtype=torch.int32, device="cuda")
    dense = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
    need = int(L.sqz_hip_encode_scratch_bytes_dict(n, total, len(dct)))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    dscratch = torch.empty(int(L.sqz_hip_decode_scratch_bytes(n, total)), dtype=torch.uint8, device="cuda")
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    fenc = F.FrameEncoder(total, WIN_BITS, BLOCK_BITS, dictionary=d_dict)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), res

    def enc_a():
        rc = L.sqz_hip_encode_blocks_dict(p(d_in), p(in_off), n, window, 0, p(d_dict), len(dct), p(slabs), p(slab_off),
                                          p(sizes), p(err), p(scratch), need, st())
        assert rc == 0, rc
        return batch.pack_blocks(slabs, slab_off, sizes, dense=dense)[1]

    def enc_b():
        return fenc.encode(d_in)

    enc_a(), enc_b()                                        # warm-up of every shape the timed window uses
    torch.cuda.synchronize()
    ea, eb = [], []
    for _ in range(a.repeats):
        ms, dense_off = timed(enc_a)
        assert int(err.abs().sum()) == 0
        ea.append(ms)
        ms, (frame, frame_bytes, status, ferr) = timed(enc_b)
        assert int(status.item()) == 0 and int(ferr.abs().sum()) == 0
        eb.append(ms)
    fb = int(frame_bytes.item())
    head = frame[:fb].cpu().numpy().tobytes()
    info = F.frame_info(head)
    packed = int(dense_off[-1].item())
    assert info["version"] == 3 and info["n_blocks"] == n and info["payload_bytes"] == packed
    assert torch.equal(frame[info["payload_off"]:fb], dense[:packed]), "frame payload differs from the packed batch"

    dframe = frame[:fb]

    def dec_a():
        rc = L.sqz_hip_decode_blocks_dict(p(dense), p(dense_off), n, p(d_dict), len(dct), p(back), p(in_off), p(err),
                                          p(dscratch), dscratch.numel(), st())
        assert rc == 0, rc
        return err

    def dec_b():
        return F.decode_frame(dframe, back, info=info, dictionary=d_dict)

    dec_a(), dec_b()
    torch.cuda.synchronize()
    da, db = [], []
    for _ in range(a.repeats):
        back.zero_()
        ms, e = timed(dec_a)
        assert int(e.abs().sum()) == 0 and torch.equal(back, d_in)
        da.append(ms)
        back.zero_()
        ms, (e, s) = timed(dec_b)
        assert int(s.item()) == 0 and int(e.abs().sum()) == 0 and torch.equal(back, d_in)
        db.append(ms)

    def pair(xa, xb):
        return {"A": stats(xa), "B": stats(xb),
                "B_minus_A_ms": round(statistics.median(xb) - statistics.median(xa), 4)}

    res = {"what": "SQZF version 3, device resident, against the batch path with the same dictionary; ranged reads "
                   "from the resident frame against the host read_range on a host copy; one process",
           "device": sqz_amd.device_info()["name"], "blocks": n, "block_bytes": bb, "win_bits": WIN_BITS,
           "dict_bytes": len(dct), "content_bytes": total, "frame_bytes": fb, "repeats": a.repeats,
           "encode": pair(ea, eb), "decode": pair(da, db), "read": {}}

    # ---- ranged reads: one aligned block; 64 KB that start inside a block and so cover 17 ----
    flat_b = flat.tobytes()
    for name, at, length in (("one_block_4K", 1000 * bb, bb), ("17_blocks_64K", 2000 * bb + 100, 65536)):
        out = torch.empty(length, dtype=torch.uint8, device="cuda")

        def rd_b():
            return F.read_frame(dframe, at, length, d_out=out, info=info, dictionary=d_dict)

        def rd_a():
            t0 = time.perf_counter()
            got = F.read_range(head, at, length, dictionary=dct)
            return (time.perf_counter() - t0) * 1e3, got

        rd_a(), rd_b()
        torch.cuda.synchronize()
        ra, rb = [], []
        for _ in range(a.repeats):
            ms, got = rd_a()
            assert got == flat_b[at:at + length]
            ra.append(ms)
            out.zero_()
            ms, (got, rerr, rstatus) = timed(rd_b)
            assert int(rstatus.item()) == 0 and got.cpu().numpy().tobytes() == flat_b[at:at + length]
            rb.append(ms)
        res["read"][name] = dict(pair(ra, rb), offset=at, length=length, covering_blocks=int(rerr.numel()),
                                 A_is="host read_range on a host copy, wall clock", B_is="read_frame, HIP event pair")
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
