"""What an SQZF frame costs on top of the batch path, measured in ONE process on the bench batch
(4096 x 256 KB Zipf, window 2^15, device resident), and one large buffer through the host calls.

  A  sqz_hip_encode_blocks + sqz_hip_pack_blocks   (today's way to a dense image; torch does the prefix sum)
  B  sqz_hip_frame_encode                          (the same streams + checksums + index, one artifact)
and the same pair for decode (sqz_hip_decode_blocks on the dense image / sqz_hip_frame_decode).  A and B
alternate after a warm-up of both; every figure is a HIP event pair on the launch stream.  The run-to-run
spread of A (max - min over its repeats) is reported next to B - A.  The checksum and index kernels' own
times come from a separate, untimed-otherwise pass with sqz_hip_set_timing(1).

Host calls: a 24 MiB slice of the same data through sqz_compress / sqz_decompress (one stream) and through
sqz_frame_compress / sqz_frame_decompress (96 blocks), wall time around calls that end in a synchronise.
The frame path must be faster in both directions (96 dependent chains against one): asserted.

    python tools/microbench/frame_bench.py [--blocks 4096] [--repeats 5] [--out profiles/frame_bench.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X


def kernel_build_id():
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "sqz_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name), "rb") as fh:
            h.update(name.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--block-bits", type=int, default=18)
    ap.add_argument("--win-bits", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-mib", type=int, default=24)
    ap.add_argument("--commit", default=os.environ.get("SQZ_COMMIT", "unknown"),
                    help="commit id the working tree sits on (recorded, not checked)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "frame_bench.py needs a GPU: there is nothing to measure without one"
    import sqz_amd
    from sqz_amd import batch, frame as F

    n, bits, wb = a.blocks, a.block_bits, a.win_bits
    bb = 1 << bits
    content = n * bb
    d_in = batch.zipf_blocks(n, bb)
    in_off = batch.uniform_offsets(n, bb)
    enc = batch.Encoder(n, content, sqz_amd.bound(bb))
    dense = torch.empty(n * sqz_amd.bound(bb), dtype=torch.uint8, device="cuda")
    fenc = F.FrameEncoder(content, wb, bits)
    torch.cuda.synchronize()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), res

    def enc_a():
        out, out_off, out_bytes, err = enc.encode(d_in, in_off, 1 << wb)
        _, off = batch.pack_blocks(out, out_off, out_bytes, dense=dense)
        return off, err

    def enc_b():
        return fenc.encode(d_in)

    enc_a(), enc_b()                                   # warm-up of every shape the timed window uses
    torch.cuda.synchronize()
    ea, eb = [], []
    for _ in range(a.repeats):
        ms, (dense_off, err) = timed(enc_a)
        assert int(err.abs().sum()) == 0
        ea.append(ms)
        ms, (frame, frame_bytes, status, ferr) = timed(enc_b)
        assert int(status.item()) == 0 and int(ferr.abs().sum()) == 0
        eb.append(ms)
    fb = int(frame_bytes.item())
    info = F.frame_info(frame[:32].cpu().numpy().tobytes())
    assert info["frame_bytes"] == fb and info["n_blocks"] == n
    # same streams: the frame's payload is the dense image
    total = int(dense_off[-1].item())
    assert total == info["payload_bytes"]
    assert torch.equal(frame[info["payload_off"]:fb], dense[:total]), "frame payload differs from the packed batch"

    batch.set_timing(True)
    batch.get_timing(reset=True)
    enc_b()
    torch.cuda.synchronize()
    ktim_enc = batch.get_timing(reset=True)
    batch.set_timing(False)

    # ---- decode ----
    d_back = torch.empty_like(d_in)
    derr = torch.zeros(n, dtype=torch.int32, device="cuda")
    dframe = frame[:fb]

    def dec_a():
        batch.decode_blocks(dense, dense_off, n, d_back, in_off, derr)
        return derr

    def dec_b():
        return F.decode_frame(dframe, d_back, info=info)

    dec_a(), dec_b()
    torch.cuda.synchronize()
    da, db = [], []
    for _ in range(a.repeats):
        d_back.zero_()
        ms, e = timed(dec_a)
        assert int(e.abs().sum()) == 0 and torch.equal(d_back, d_in)
        da.append(ms)
        d_back.zero_()
        ms, (e, st) = timed(dec_b)
        assert int(st.item()) == 0 and int(e.abs().sum()) == 0 and torch.equal(d_back, d_in)
        db.append(ms)
    batch.set_timing(True)
    batch.get_timing(reset=True)
    dec_b()
    torch.cuda.synchronize()
    ktim_dec = batch.get_timing(reset=True)
    batch.set_timing(False)

    def summary(xa, xb, ktim):
        crc_ms, crc_launches = ktim.get("crc32_blocks_kernel", (0.0, 0))
        idx_ms = ktim.get("frame_index_kernel", (0.0, 0))[0]
        med_a, med_b = statistics.median(xa), statistics.median(xb)
        return {"A_ms": [round(x, 3) for x in xa], "B_ms": [round(x, 3) for x in xb],
                "A_median_ms": round(med_a, 3), "B_median_ms": round(med_b, 3),
                "B_minus_A_ms": round(med_b - med_a, 3), "A_spread_ms": round(max(xa) - min(xa), 3),
                "crc32_blocks_kernel_ms": round(crc_ms, 4), "crc32_launches": crc_launches,
                "frame_index_kernel_ms": round(idx_ms, 4),
                "crc_share_of_A_percent": round(100.0 * crc_ms / med_a, 3),
                # the content is read once; the index adds 8 bytes per block
                "crc_GBps": round((content + 8 * n) / (crc_ms * 1e-3) / 1e9, 1) if crc_ms > 0 else None,
                "crc_share_of_hbm_peak_percent": round(100.0 * (content + 8 * n) / (crc_ms * 1e-3) / HBM_PEAK, 2)
                if crc_ms > 0 else None}

    res = {"what": "SQZF frame against the batch path, one process, HIP events",
           "device": sqz_amd.device_info()["name"], "commit": a.commit, "kernel_build_id": kernel_build_id(),
           "blocks": n, "block_bytes": bb, "win_bits": wb, "content_bytes": content, "frame_bytes": fb,
           "repeats": a.repeats,
           "encode": summary(ea, eb, ktim_enc), "decode": summary(da, db, ktim_dec),
           "crc_bound": "instruction issue: the bitwise reduction spends 3 vector operations per message bit "
                        "(v_bfe_i32, v_lshrrev_b32, v_bitop3_b32); the HBM bound of one read of the content at "
                        "8 TB/s is content_bytes / 8e12 s"}
    res["encode"]["hbm_bound_ms"] = res["decode"]["hbm_bound_ms"] = round(content / HBM_PEAK * 1e3, 4)

    # ---- one large buffer through the host calls ----
    host = d_in[:a.host_mib << 20].cpu().numpy().tobytes()
    del enc, fenc, dense, d_back
    torch.cuda.empty_cache()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    sqz_amd.compress(host[:1 << 16], wb), F.compress_frame(host[:1 << 20], wb, bits)        # warm-up
    one_c_ms, comp = wall(lambda: sqz_amd.compress(host, win_bits=wb, header=True))
    frm_c_ms, hframe = wall(lambda: F.compress_frame(host, wb, bits))
    one_d_ms, back1 = wall(lambda: sqz_amd.decompress(comp, header=True))
    frm_d_ms, back2 = wall(lambda: F.decompress_frame(hframe))
    assert back1 == host and back2 == host
    res["host_one_buffer"] = {"bytes": len(host), "blocks_in_frame": F.frame_info(hframe)["n_blocks"],
                              "sqz_compress_ms": round(one_c_ms, 1), "sqz_frame_compress_ms": round(frm_c_ms, 1),
                              "sqz_decompress_ms": round(one_d_ms, 1), "sqz_frame_decompress_ms": round(frm_d_ms, 1),
                              "compress_ratio_one_over_frame": round(one_c_ms / frm_c_ms, 2),
                              "decompress_ratio_one_over_frame": round(one_d_ms / frm_d_ms, 2),
                              "stream_bytes": len(comp), "frame_bytes": len(hframe)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    assert frm_c_ms < one_c_ms and frm_d_ms < one_d_ms, "the frame path must beat one stream in both directions"


if __name__ == "__main__":
    main()
