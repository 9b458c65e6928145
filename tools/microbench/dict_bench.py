"""What a shared dictionary (SQZF version 3) costs per step and buys in bytes, in one GPU visit.

  1  the step: 16,384 blocks of 4 KB cut from confucius.txt behind its first 32,767 bytes, window 2^15, device
     resident, encoded and decoded WITHOUT a dictionary (side A: sqz_hip_encode_blocks / sqz_hip_decode_blocks) and
     WITH those 32,767 bytes as the dictionary (side B: the _dict calls), A and B alternating `--repeats` times after
     a warm-up of each.  Every figure is a HIP event pair on the launch stream; median and spread (max - min).
  2  the new kernels: stage 1 alone (sqz_hip_lz77_blocks_parse / sqz_hip_lz77_blocks_dict) with the library's kernel
     timing on.  sqz_hip_timing has no free slot, so dict_match_kernel is timed here: the call's event pair minus
     the three timed kernels is launch gaps on side A and launch gaps + dict_match_kernel (+ a one-thread offsets
     kernel) on side B.  The dictionary's sort runs under the index_sort slot: side B's slot minus side A's.
  3  the corpus table: payload bytes with and without a dictionary per file and block size (the dictionary is the
     first half of the file, at most 32,767 bytes; the content is what follows it, x64.elf's cut to 65,536 bytes),
     through the host calls, and the same figures from the model (tests/dict_model.py): they must be equal to the
     byte.  The model is slow brute force on the CPU; --model-cache keeps its figures in a file.

    python tools/microbench/dict_bench.py [--out profiles/dict_bench.json] [--corpus-out profiles/dict_corpus.json]
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

WINDOW = 1 << 15
DICT_MAX = WINDOW - 1
CORPUS = (("confucius.txt", None, 1024), ("confucius.txt", None, 4096), ("confucius.txt", None, 16384),
          ("laozi.txt", None, 4096), ("x64.elf", 65536, 4096))


def stats(xs):
    return {"ms": [round(x, 4) for x in xs], "median_ms": round(statistics.median(xs), 4),
            "spread_ms": round(max(xs) - min(xs), 4)}


def split(name, cut):
    import oracle_lib as O
    data = O.corpus(name)
    d = min(len(data) // 2, DICT_MAX)
    content = data[d:] if cut is None else data[d:d + cut]
    return data[:d], content


def corpus_table(model_cache):
    from sqz_amd import batch
    cache = {}
    if model_cache and os.path.exists(model_cache):
        with open(model_cache) as fh:
            cache = json.load(fh)
    rows = []
    for name, cut, bb in CORPUS:
        dct, content = split(name, cut)
        blocks = [content[k:k + bb] for k in range(0, len(content), bb)]
        plain, err = batch.encode_blocks_host(blocks, WINDOW)
        assert not err.any()
        with_d, err = batch.encode_blocks_host(blocks, WINDOW, dictionary=dct)
        assert not err.any()
        lazy_d, err = batch.encode_blocks_host(blocks, WINDOW, parse="lazy", dictionary=dct)
        assert not err.any()
        back, err = batch.decode_blocks_host(with_d, [len(b) for b in blocks], dictionary=dct)
        assert not err.any() and back == blocks
        key = f"{name}:{len(content)}:{bb}"
        if key not in cache:
            import dict_model as DM
            cache[key] = [sum(len(DM.stream(b"", b, WINDOW)) for b in blocks),
                          sum(len(DM.stream(dct, b, WINDOW)) for b in blocks)]
        row = {"file": name, "content_bytes": len(content), "dict_bytes": len(dct), "block_bytes": bb,
               "blocks": len(blocks), "payload_no_dict": sum(map(len, plain)), "payload_dict": sum(map(len, with_d)),
               "payload_dict_lazy": sum(map(len, lazy_d)), "model_no_dict": cache[key][0], "model_dict": cache[key][1]}
        row["ratio"] = round(row["payload_dict"] / row["payload_no_dict"], 3)
        assert (row["payload_no_dict"], row["payload_dict"]) == (row["model_no_dict"], row["model_dict"]), row
        rows.append(row)
        print("[corpus]", json.dumps(row), flush=True)
    if model_cache:
        with open(model_cache, "w") as fh:
            json.dump(cache, fh)
    return rows


def bench_blocks(n):
    """dictionary, n blocks of 4 KB cut from the text behind it: every block another stretch, eight bytes of it its number"""
    import numpy as np
    dct, tail = split("confucius.txt", None)
    bb = 4096
    a = np.frombuffer(tail, np.uint8)
    out = np.empty((n, bb), np.uint8)
    for k in range(n):
        at = (k * 1237) % (len(a) - bb)
        out[k] = a[at:at + bb]
        out[k, 2000:2008] = np.frombuffer(k.to_bytes(8, "little"), np.uint8)
    return dct, out.reshape(-1), bb


def step_bench(n, repeats):
    import numpy as np
    import torch
    from sqz_amd import _native as N
    L = N.lib()
    dct, flat, bb = bench_blocks(n)
    total = n * bb
    d_in = torch.from_numpy(flat.copy()).cuda()
    d_dict = torch.from_numpy(np.frombuffer(dct, np.uint8).copy()).cuda()
    in_off = torch.arange(0, (n + 1) * bb, bb, dtype=torch.int64, device="cuda")
    cap = int(L.sqz_bound(bb))
    out_off = torch.arange(0, (n + 1) * cap, cap, dtype=torch.int64, device="cuda")
    out = {s: torch.empty(n * cap, dtype=torch.uint8, device="cuda") for s in "AB"}
    out_bytes = {s: torch.zeros(n, dtype=torch.int64, device="cuda") for s in "AB"}
    err = torch.zeros(n, dtype=torch.int32, device="cuda")
    need_a = int(L.sqz_hip_encode_scratch_bytes(n, total))
    need_b = int(L.sqz_hip_encode_scratch_bytes_dict(n, total, len(dct)))
    scratch = torch.empty(need_b, dtype=torch.uint8, device="cuda")
    dscratch = torch.empty(int(L.sqz_hip_decode_scratch_bytes(n, total)), dtype=torch.uint8, device="cuda")
    back = torch.empty(total, dtype=torch.uint8, device="cuda")
    toks = torch.empty(total + 64, dtype=torch.int32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = need_b - need_a

    def enc(side):
        if side == "A":
            rc = L.sqz_hip_encode_blocks(p(d_in), p(in_off), n, WINDOW, p(out["A"]), p(out_off), p(out_bytes["A"]), p(err),
                                         p(scratch), need_a, st())
        else:
            rc = L.sqz_hip_encode_blocks_dict(p(d_in), p(in_off), n, WINDOW, 0, p(d_dict), len(dct), p(out["B"]), p(out_off),
                                              p(out_bytes["B"]), p(err), p(scratch), need_b, st())
        assert rc == 0, rc

    def dec(side):
        if side == "A":
            rc = L.sqz_hip_decode_blocks(p(out["A"]), p(out_off), n, p(back), p(in_off), p(err), p(dscratch),
                                         dscratch.numel(), st())
        else:
            rc = L.sqz_hip_decode_blocks_dict(p(out["B"]), p(out_off), n, p(d_dict), len(dct), p(back), p(in_off), p(err),
                                              p(dscratch), dscratch.numel(), st())
        assert rc == 0, rc

    def stage1(side):
        if side == "A":
            rc = L.sqz_hip_lz77_blocks_parse(p(d_in), p(in_off), n, WINDOW, p(toks), p(counts), 1, 0, p(scratch),
                                             8 * (total + 64), st())
        else:
            rc = L.sqz_hip_lz77_blocks_dict(p(d_in), p(in_off), n, WINDOW, p(toks), p(counts), 1, 0, p(d_dict), len(dct),
                                            p(scratch), idx + 8 * (total + 64), st())
        assert rc == 0, rc

    def timed(fn, side):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(side)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    res = {"blocks": n, "block_bytes": bb, "window": WINDOW, "dict_bytes": len(dct), "repeats": repeats}
    for side in "AB":                                       # warm-up, and the round trip of both sides
        enc(side)
        back.zero_()
        dec(side)
        torch.cuda.synchronize()
        assert not err.cpu().numpy().any() and torch.equal(back, d_in), side
        res["payload_" + side] = int(out_bytes[side].sum().item())
    times = {k: [] for k in ("encode_A", "encode_B", "decode_A", "decode_B")}
    for _ in range(repeats):
        for side in "AB":
            times["encode_" + side].append(timed(enc, side))
        for side in "AB":
            times["decode_" + side].append(timed(dec, side))
    res.update({k: stats(v) for k, v in times.items()})
    # stage 1 with the library's kernel timing on
    from sqz_amd import batch
    s1 = {s: {"call": [], "sort": [], "match": [], "parse": [], "rest": []} for s in "AB"}
    batch.set_timing(True)
    for side in "AB":
        stage1(side)
    torch.cuda.synchronize()
    batch.get_timing()
    for _ in range(repeats):
        for side in "AB":
            ms = timed(stage1, side)
            t = batch.get_timing()
            k = {name: t.get(name + "_kernel", (0.0, 0))[0] for name in ("index_sort", "index_match", "index_parse")}
            s1[side]["call"].append(ms)
            s1[side]["sort"].append(k["index_sort"])
            s1[side]["match"].append(k["index_match"])
            s1[side]["parse"].append(k["index_parse"])
            s1[side]["rest"].append(ms - sum(k.values()))
    batch.set_timing(False)
    res["stage1"] = {s: {k: stats(v) for k, v in s1[s].items()} for s in "AB"}
    med = lambda s, k: res["stage1"][s][k]["median_ms"]
    res["dict_match_kernel_ms"] = round(med("B", "rest") - med("A", "rest"), 4)
    res["dict_sort_ms"] = round(med("B", "sort") - med("A", "sort"), 4)
    res["index_match_kernel_ms"] = med("B", "match")
    res["encode_cost_ms"] = round(res["encode_B"]["median_ms"] - res["encode_A"]["median_ms"], 4)
    res["decode_cost_ms"] = round(res["decode_B"]["median_ms"] - res["decode_A"]["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--corpus-out", default=None)
    ap.add_argument("--model-cache", default=None)
    ap.add_argument("--skip-corpus", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    import sqz_amd
    dev = sqz_amd.device_info()["name"]
    res = step_bench(a.blocks, a.repeats)
    res["device"] = dev
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    if not a.skip_corpus:
        rows = corpus_table(a.model_cache)
        if a.corpus_out:
            with open(a.corpus_out, "w") as fh:
                json.dump({"device": dev, "window": WINDOW, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
