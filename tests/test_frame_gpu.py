"""GPU: SQZF frames through the C ABI of libsqz_amd.so -- the checksum kernel against zlib.crc32, frames byte for
byte against the independent writer (tests/frame_writer.py: struct + zlib + the CPU oracle, and the compiled
reference where oracle/_ref exists), round trips of the host and the device flavour, refusals and ranged reads.

Corruption tests feed malformed DATA to hardened code: each shows that the refusal is an errno.
Nothing here reads /root/reference: the GPU box does not have it."""
import ctypes as C
import errno
import os
import random
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import frame_writer as W
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BB = 1 << 18


@pytest.fixture(scope="module")
def F():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import frame
    return frame


@pytest.fixture(scope="module")
def L():
    from sqz_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def big(F):
    """64 Zipf blocks of 256 KB as one 16 MiB buffer, its frame at window 2^15 and the streams of the batch path"""
    from sqz_amd import batch
    import torch
    data = batch.zipf_blocks(64, BB).cpu().numpy().tobytes()
    torch.cuda.synchronize()
    assert data[:BB] == O.zipf_block(0, BB)
    frame = F.compress_frame(data, 15, 18)
    streams, err = batch.encode_blocks_host(W.blocks_of(data, 18), 1 << 15)
    assert not err.any()
    return data, frame, streams


def dev(t):
    import torch
    return torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda() if len(t) else torch.empty(0, dtype=torch.uint8, device="cuda")


def encode_on_device(F, data, wb, bits):
    enc = F.FrameEncoder(len(data), wb, bits)
    enc.encode(dev(data))
    return enc.result(), enc


def decode_on_device(F, frame, pattern=0x5A, info=None, trailing=0):
    """-> (bytes of d_out, err list, status); d_out is pre-filled with `pattern`"""
    import torch
    info = F.frame_info(frame[:32]) if info is None else info
    d_frame = dev(frame + bytes(trailing))
    d_out = torch.full((max(info["content_bytes"], 1),), pattern, dtype=torch.uint8, device="cuda")
    err, status = F.decode_frame(d_frame, d_out, info=info)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().tobytes()[:info["content_bytes"]], err.cpu().tolist(), int(status.item())


# ---------------------------------------------------------------- 6. the checksum kernel
def test_crc32_blocks_against_zlib(F):
    import torch
    lengths = [0, 1, 3, 63, 64, 65, 255, 4095, 4096, 4097, 70001, 262144, (1 << 20) + 3]
    raw = np.random.default_rng(11).integers(0, 256, (1 << 20) + 64, dtype=np.uint8)
    d = torch.from_numpy(raw).cuda()
    assert d.data_ptr() % 16 == 0
    pairs = [(s, s + n) for n in lengths for s in range(18)]
    # every range in a launch of its own (a launch of one range is cut into parts) ...
    for a, b in pairs[::7] + [(17, 17 + (1 << 20) + 3), (5, 5 + 262144)]:
        off = torch.tensor([a, b], dtype=torch.int64, device="cuda")
        got = int(F.crc32_blocks(d, off).cpu().numpy().view(np.uint32)[0])
        assert got == zlib.crc32(raw[a:b].tobytes()), (a, b)
    # ... and all of them as one ragged batch: ranges need not be ordered or disjoint, only off[b] .. off[b+1]
    flat = []
    for a, b in pairs:
        flat += [a, b]
    off = torch.tensor(flat + [flat[-1]], dtype=torch.int64, device="cuda")       # range 2k is pairs[k]
    got = F.crc32_blocks(d, off).cpu().numpy().view(np.uint32)[0::2].tolist()
    assert got == [zlib.crc32(raw[a:b].tobytes()) for a, b in pairs]
    assert F.crc32_blocks(d, torch.zeros(1, dtype=torch.int64, device="cuda")).numel() == 0      # n = 0


def test_crc32_of_one_64_mib_range_and_of_a_4096_block_batch(F):
    import torch
    from sqz_amd import batch
    d = batch.zipf_blocks(4096, BB)
    host = d.cpu().numpy()
    one = torch.tensor([3, 3 + (64 << 20)], dtype=torch.int64, device="cuda")
    assert int(F.crc32_blocks(d, one).cpu().numpy().view(np.uint32)[0]) == zlib.crc32(host[3:3 + (64 << 20)].tobytes())
    got = F.crc32_blocks(d, batch.uniform_offsets(4096, BB)).cpu().numpy().view(np.uint32).tolist()
    assert got == [zlib.crc32(host[b * BB:(b + 1) * BB].tobytes()) for b in range(4096)]


# ---------------------------------------------------------------- 7. byte-exact frames
@pytest.mark.parametrize("name", W.CASE_IDS)
def test_frames_equal_the_independent_writer(F, name):
    _, _, wb, bits, _ = next(c for c in W.CASES if c[0] == name)
    data, want = W.case_data(name), W.case_frame(name)
    got = F.compress_frame(data, wb, bits)
    assert got == want
    on_device, _ = encode_on_device(F, data, wb, bits)
    assert on_device == got
    # 9. and back, both flavours, also with something behind the frame
    assert F.decompress_frame(got) == data
    assert F.decompress_frame(got + b"trailing record") == data
    back, err, status = decode_on_device(F, got, trailing=40)
    assert status == 0 and not any(err) and back == data


@pytest.mark.skipif(O.REF is None, reason="oracle/_ref (the compiled reference) is not built here")
@pytest.mark.parametrize("wb", [12, 15])
def test_frames_equal_the_writer_over_the_compiled_reference(F, wb):
    data = O.corpus("laozi.txt")
    want = W.write_frame(data, wb, 12, encode=lambda blk: O.ref_compress(blk, wb, header=False))
    assert F.compress_frame(data, wb, 12) == want


def test_golden_frame(F):
    with open(os.path.join(O.GOLD, "laozi.txt.w15.b12.sqzf"), "rb") as fh:
        gold = fh.read()
    data = O.corpus("laozi.txt")
    assert F.compress_frame(data, 15, 12) == gold
    assert encode_on_device(F, data, 15, 12)[0] == gold
    assert F.decompress_frame(gold) == data


# ---------------------------------------------------------------- 8. full size
def test_full_size_frame(F, big):
    data, frame, streams = big
    fi = F.frame_info(frame)
    assert fi["n_blocks"] == 64 and fi["content_bytes"] == len(data) and fi["frame_bytes"] == len(frame)
    assert frame == W.assemble(data, 15, 18, streams)       # streams of sqz_encode_blocks, CRCs of zlib, framing
    assert encode_on_device(F, data, 15, 18)[0] == frame
    assert F.decompress_frame(frame) == data
    back, err, status = decode_on_device(F, frame)
    assert status == 0 and not any(err) and back == data


# ---------------------------------------------------------------- 9. round trips
def _mixed(nbytes, seed):
    rng = random.Random(seed)
    text = O.corpus("confucius.txt")
    out = bytearray()
    while len(out) < nbytes:
        k = rng.randrange(3)
        if k == 0:
            a = rng.randrange(len(text) - 5000)
            out += text[a:a + rng.randrange(100, 5000)]
        elif k == 1:
            out += O.zipf_block(rng.randrange(1000), rng.randrange(100, 4000))
        else:
            out += bytes([rng.randrange(256)]) * rng.randrange(1, 900)
    return bytes(out[:nbytes])


@pytest.mark.parametrize("bits,nbytes", [(12, 4096), (12, 4097), (12, 50001), (16, 65536), (16, 65537), (16, 300007),
                                         (18, (1 << 18) + 1), (20, (3 << 20) + 12345)])
def test_round_trips(F, bits, nbytes):
    data = _mixed(nbytes, bits * 1000 + nbytes % 997)
    frame = F.compress_frame(data, 13, bits)
    assert F.frame_info(frame)["n_blocks"] == -(-nbytes // (1 << bits))
    assert F.decompress_frame(frame) == data
    on_device, _ = encode_on_device(F, data, 13, bits)
    assert on_device == frame
    back, err, status = decode_on_device(F, frame)
    assert status == 0 and not any(err) and back == data


def test_round_trip_with_16_mib_blocks(F, big):
    data = big[0] + b"one more block"
    frame = F.compress_frame(data, 15, 24)
    assert F.frame_info(frame)["n_blocks"] == 2
    assert F.decompress_frame(frame) == data
    back, err, status = decode_on_device(F, frame)
    assert status == 0 and not any(err) and back == data


def test_two_host_passes_give_the_same_frame(F, big, monkeypatch):
    data, frame, _ = big
    monkeypatch.setenv("SQZ_FRAME_PASS_BYTES", str(5 * BB))        # 64 blocks in 13 passes, the last one short
    assert F.compress_frame(data, 15, 18) == frame
    assert F.decompress_frame(frame) == data
    assert F.read_range(frame, 3 * BB + 5, 9 * BB) == data[3 * BB + 5:12 * BB + 5]


# ---------------------------------------------------------------- 10. refusals
def _decompress_raw(L, frame, capacity=None, guard=64):
    fi = W.fields(frame)
    cap = fi["content_bytes"] if capacity is None else capacity
    store = bytearray(b"\xC3" * (cap + guard))
    out = (C.c_uint8 * (cap + guard)).from_buffer(store)
    errs = (C.c_int32 * max(fi["n_blocks"], 1))()
    n = C.c_uint64(0)
    rc = L.sqz_frame_decompress(frame, len(frame), out, cap, C.byref(n), errs)
    del out
    raw = bytes(store)
    return rc, raw[:cap], raw[cap:], list(errs)[:fi["n_blocks"]], n.value


def test_a_flipped_payload_bit_fails_its_block_only(F, L, big):
    data, frame, streams = big
    fi = F.frame_info(frame)
    k = 37
    at = fi["payload_off"] + sum(len(s) for s in streams[:k]) + len(streams[k]) // 2
    bad = bytearray(frame)
    bad[at] ^= 0x04
    rc, out, guard, errs, _ = _decompress_raw(L, bytes(bad))
    assert rc != 0 and errs[k] != 0 and rc == errs[k]
    assert [e for b, e in enumerate(errs) if b != k] == [0] * 63
    assert out[:k * BB] == data[:k * BB] and out[(k + 1) * BB:] == data[(k + 1) * BB:]
    assert guard == b"\xC3" * 64
    with pytest.raises(F.SqzError) as ei:
        F.decompress_frame(bytes(bad))
    assert ei.value.block_errors == errs
    back, derr, status = decode_on_device(F, bytes(bad))
    assert status == 0 and derr == errs
    # ranged reads: a range that does not touch block k succeeds, one that does fails
    assert F.read_range(bytes(bad), (k + 1) * BB, 2 * BB + 17) == data[(k + 1) * BB:(k + 3) * BB + 17]
    assert F.read_range(bytes(bad), 0, k * BB) == data[:k * BB]
    with pytest.raises(F.SqzError):
        F.read_range(bytes(bad), k * BB - 1, 2)


def test_a_flipped_stored_checksum_is_eilseq_with_the_right_bytes(F, L, big):
    data, frame, _ = big
    k = 5
    bad = bytearray(frame)
    bad[32 + 8 * k + 4] ^= 0x80
    bad = W.reseal(bad)                                     # the index itself is intact: only block k's bytes "differ"
    rc, out, _, errs, n = _decompress_raw(L, bad)
    assert rc == errno.EILSEQ and errs == [0] * k + [errno.EILSEQ] + [0] * (63 - k)
    assert out == data and n == len(data)
    back, derr, status = decode_on_device(F, bad)
    assert status == 0 and derr == errs and back == data


def test_index_corruptions_are_refused_by_both_flavours(F, L):
    data, frame = W.case_data("laozi_w15_b12"), W.case_frame("laozi_w15_b12")
    good = W.fields(frame)
    for name, bad, head_errno, full_errno in W.refusals(frame):
        rc, out, guard, errs, _ = _decompress_raw(L, bad, capacity=good["content_bytes"])
        assert rc == full_errno, name
        assert out == b"\xC3" * len(out) and guard == b"\xC3" * 64, name       # refused before anything is delivered
        # the device flavour with what a caller has: the header's figures where the header alone parses
        info = dict(good)
        if head_errno == 0:
            info.update(W.fields(bad))
        back, derr, status = decode_on_device(F, bad, info=info)
        want = full_errno if head_errno == 0 else errno.EINVAL
        assert status == want and derr == [want] * good["n_blocks"], name
        assert back == b"\x5A" * len(back), name                                # d_out untouched


def test_truncated_avail(F, L):
    frame = W.case_frame("confucius_w15_b14")
    fi = W.fields(frame)
    out = (C.c_uint8 * fi["content_bytes"])()
    for cut in (31, 40, fi["payload_off"] - 1, fi["payload_off"], len(frame) - 8, len(frame) - 1):
        assert L.sqz_frame_decompress(frame, cut, out, len(out), None, None) == errno.E2BIG, cut
    # device flavour: the payload does not lie inside avail
    import torch
    d_frame = dev(frame)
    d_out = torch.full((fi["content_bytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    err, status = F.decode_frame(d_frame[:len(frame) - 8], d_out, info=fi)
    torch.cuda.synchronize()
    assert int(status.item()) == errno.E2BIG and err.cpu().tolist() == [errno.E2BIG] * fi["n_blocks"]
    assert bool((d_out == 0x5A).all())
    with pytest.raises(F.SqzError) as ei:                    # not even the index: refused at the call
        F.decode_frame(d_frame[:32 + 8], d_out, info=fi)
    assert ei.value.errno == errno.E2BIG


def test_capacity_too_small(F, L):
    import torch
    data, frame = W.case_data("confucius_w15_b14"), W.case_frame("confucius_w15_b14")
    for cap in (len(frame) - 1, len(frame) - 4096, 40, 0):
        store = bytearray(b"\xC3" * (cap + 64))
        buf = (C.c_uint8 * (cap + 64)).from_buffer(store)
        n = C.c_uint64(0)
        assert L.sqz_frame_compress(data, len(data), 15, 14, buf, cap, C.byref(n)) == errno.E2BIG, cap
        del buf
        assert n.value == len(frame) and bytes(store[cap:]) == b"\xC3" * 64
    enc = F.FrameEncoder(len(data), 15, 14)
    enc.frame.fill_(0xC3)
    enc.capacity = len(frame) - 8
    enc.encode(dev(data))
    torch.cuda.synchronize()
    assert int(enc.status.item()) == errno.E2BIG and int(enc.frame_bytes.item()) == len(frame)
    assert bool((enc.frame == 0xC3).all())                   # nothing written at all, so nothing beyond capacity
    enc.capacity = len(frame)                                # exactly enough
    enc.encode(dev(data))
    assert enc.result() == frame and bool((enc.frame[len(frame):] == 0xC3).all())
    rc, out, guard, errs, n = _decompress_raw(L, frame, capacity=len(data) - 1)
    assert rc == errno.E2BIG and n == len(data) and out == b"\xC3" * len(out) and guard == b"\xC3" * 64


# ---------------------------------------------------------------- 11. ranged reads
def test_read_range(F, big):
    data, frame, _ = big
    rng = random.Random(2024)
    n = len(data)
    pairs = [(0, 0), (n, 0), (0, n), (n - 1, 1), (BB - 1, 2), (BB, BB), (5 * BB + 7, 0)]
    while len(pairs) < 200:
        kind = rng.randrange(4)
        if kind == 0:                                       # inside one block
            b = rng.randrange(64)
            a = rng.randrange(BB)
            pairs.append((b * BB + a, rng.randrange(BB - a)))
        elif kind == 1:                                     # across two
            b = rng.randrange(63)
            pairs.append((b * BB + rng.randrange(BB), BB))
        elif kind == 2:                                     # anything
            a = rng.randrange(n)
            pairs.append((a, rng.randrange(min(n - a, 6 * BB) + 1)))
        else:                                               # long
            a = rng.randrange(n // 8)
            pairs.append((a, rng.randrange(n - a + 1)))
    for off, length in pairs:
        assert F.read_range(frame, off, length) == data[off:off + length], (off, length)
    for off, length in ((n + 1, 0), (n, 1), (0, n + 1), (1 << 63, 1 << 63)):
        with pytest.raises(F.SqzError) as ei:
            F.read_range(frame, off, length)
        assert ei.value.errno == errno.EINVAL


def test_a_one_block_range_decodes_one_block(F, big):
    from sqz_amd import batch
    data, frame, _ = big
    F.read_range(frame, 0, 16)                              # warm
    batch.set_timing(True)
    try:
        batch.get_timing(reset=True)
        assert F.read_range(frame, 20 * BB + 100, 1000) == data[20 * BB + 100:20 * BB + 1100]
        one = batch.get_timing(reset=True)
        assert F.decompress_frame(frame) == data
        full = batch.get_timing(reset=True)
    finally:
        batch.set_timing(False)
    print("entropy_decode_kernel: one-block range", one["entropy_decode_kernel"], "whole frame", full["entropy_decode_kernel"])
    assert one["entropy_decode_kernel"][1] == 1 and full["entropy_decode_kernel"][1] == 1
    assert one["entropy_decode_kernel"][0] < full["entropy_decode_kernel"][0]
    assert "crc32_blocks_kernel" in one and "frame_index_kernel" in one


# ---------------------------------------------------------------- 12. the file tool
def test_file_tool(F, tmp_path):
    src = os.path.join(O.CORPUS, "x64.elf")
    packed, back = str(tmp_path / "x64.sqzf"), str(tmp_path / "x64.back")
    run = lambda *a: subprocess.run([sys.executable, "-m", "sqz_amd.frame", *a], cwd=ROOT, capture_output=True,
                                    text=True, timeout=600)
    r = run("c", src, packed, "--win-bits", "12", "--block-bits", "16")
    assert r.returncode == 0, r.stdout + r.stderr
    with open(packed, "rb") as fh:
        assert fh.read() == W.case_frame("x64_w12_b16")
    r = run("d", packed, back)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(back, "rb") as fh:
        assert fh.read() == O.corpus("x64.elf")
    r = run("info", packed)
    assert r.returncode == 0, r.stdout + r.stderr
    said = {k: int(v) for k, v in (line.split(": ") for line in r.stdout.strip().splitlines())}
    assert said == W.fields(W.case_frame("x64_w12_b16"))
