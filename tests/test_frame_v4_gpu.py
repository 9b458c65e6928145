"""GPU: SQZF version 4 (the byte-shuffle filter) on gfx950 -- the standalone shuffle call against numpy, frames byte for
byte against the independent writer (tests/frame_writer_v4.py) and the golden frame, host and device-resident flavours,
decode, ranged reads, damage, and every older call's refusal.  The contents are the 16,389-byte closed-form inputs of
the payload table (four blocks of 4 KB and a ragged one of 5 bytes) and a few tiny ones; the writer's frames are
computed once per process (functools.lru_cache in the writer)."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import frame_writer_v4 as W4
import oracle_lib as O
from test_frame_emu import LENGTHS

pytestmark = pytest.mark.gpu

E = errno
GUARD = 0x5A
TILE_BYTES = 8192
INPUT = {2: "u32_ramp", 4: "u32_ramp", 8: "f32_sine"}        # 16389 bytes each (the i16 input of the table has 12000)


@pytest.fixture(scope="module")
def F():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import frame
    return frame


def dev(b: bytes, slack: int = 64):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) + bytes(slack), np.uint8).copy()).cuda()


def filled(n: int):
    import torch
    return torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")


def host(t):
    return t.cpu().numpy()


def sync():
    import torch
    torch.cuda.synchronize()


def content(e: int) -> bytes:
    return W4.figure_input(INPUT[e])


# ---------------------------------------------------------------- the standalone call
def lengths_for(e):
    t = TILE_BYTES // e
    return sorted(set(LENGTHS + list(range(2 * e + 2)) + [(t - 1) * e, t * e, (t + 1) * e, t * e + e - 1]))


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_shuffle_blocks_equals_numpy(F, e, inverse):
    import torch
    lens = lengths_for(e) + [0, 3 * 1024 * 1024 + 5]         # an empty range among them; one range that many workgroups share
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(cuts[-1])
    data = np.random.default_rng(e).integers(0, 256, total, dtype=np.uint8)
    fn = W4.unshuffle if inverse else W4.shuffle
    want = b"".join(fn(data[a:b].tobytes(), e) for a, b in zip(cuts, cuts[1:]))
    off = torch.from_numpy(cuts).cuda()
    for mis in (0, 1, 7, 16):                                # the tensor sliced at an offset: every base misaligned
        out_mis = (5 * mis + 3) % 17
        d_in = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        d_in[mis:mis + total] = torch.from_numpy(data).cuda()
        d_out = filled(total + 64)
        got = F.shuffle_blocks(d_in[mis:mis + total], off, e, inverse, d_out=d_out[out_mis:out_mis + total])
        sync()
        assert got.data_ptr() == d_out.data_ptr() + out_mis
        h = host(d_out)
        assert h[out_mis:out_mis + total].tobytes() == want, (e, inverse, mis)
        assert (h[:out_mis] == GUARD).all() and (h[out_mis + total:] == GUARD).all(), (e, inverse, mis)
    back = F.shuffle_blocks(F.shuffle_blocks(d_in[16:16 + total], off, e, inverse), off, e, not inverse)
    sync()
    assert host(back).tobytes() == data.tobytes()
    with pytest.raises(ValueError):
        F.shuffle_blocks(d_in, off, 3)


# ---------------------------------------------------------------- frames, byte for byte
def encode_dev(F, data, wb, bits, e, store, parse, capacity=None):
    enc = F.FrameEncoder(len(data), wb, bits, capacity=capacity, store=store, parse=parse, shuffle=e)
    enc.frame.fill_(GUARD)
    frame, frame_bytes, status, err = enc.encode(dev(data), len(data))
    sync()
    return enc, host(frame), int(frame_bytes.item()), int(status.item()), host(err)


def check_frame(F, data, wb, bits, e, store, parse):
    import sqz_amd
    want = W4.write_frame(data, wb, bits, e, store, parse == "lazy")
    what = (len(data), wb, bits, e, store, parse)
    got = sqz_amd.compress_frame(data, wb, bits, store=store, parse=parse, shuffle=e)       # the host flavour
    assert got == want, (what, next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), None))
    enc, frame, frame_bytes, status, err = encode_dev(F, data, wb, bits, e, store, parse)  # the device-resident one
    assert status == 0 and not err.any() and frame_bytes == len(want), what
    assert enc.capacity == F.frame_bound(len(data), bits, store, shuffle=e) >= len(want), what
    assert frame[:len(want)].tobytes() == want and (frame[len(want):] == GUARD).all(), what
    # ... and back: host flavour, then the resident frame into a tensor between guard bytes
    assert sqz_amd.decompress_frame(want) == data, what
    d_out = filled(len(data) + 32)
    derr, dstatus = F.decode_frame(enc.frame[:max(len(want), 1)], d_out)
    sync()
    assert int(dstatus.item()) == 0 and not host(derr).any(), what
    assert host(d_out)[:len(data)].tobytes() == data and (host(d_out)[len(data):] == GUARD).all(), what
    return want


@pytest.mark.parametrize("parse", ["greedy", "lazy"])
@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("e", W4.ELEMS)
def test_frames_equal_the_writer_and_come_back(F, e, store, parse):
    data = content(e)                                        # 16389 bytes: the last block has 5
    want = check_frame(F, data, 15, 12, e, store, parse)
    blk = W4.blocks(want)
    assert len(blk) == 5 and blk[4]["content_bytes"] == 5
    if store and e == 8:
        assert blk[4]["stored"] == 1                         # smaller than one element: nothing to shuffle, stored
    if parse == "greedy":
        for n in (0, 1, e - 1, e, 4096, 4097):
            check_frame(F, data[:n], 12, 12, e, store, parse)
    assert len(W4.write_frame(b"", 12, 12, e, store)) == 48


def test_golden_frame_block_bits_13_and_shuffle_0(F):
    import sqz_amd
    with open(os.path.join(O.GOLD, "ramp_u32.w15.b12.e4.sqzf"), "rb") as fh:
        golden = fh.read()
    data = W4.figure_input("u32_ramp")
    assert sqz_amd.compress_frame(data, 15, 12, shuffle=4) == golden       # the reference's own streams
    assert encode_dev(F, data, 15, 12, 4, False, "greedy")[1][:len(golden)].tobytes() == golden
    assert sqz_amd.decompress_frame(golden) == data and sqz_amd.frame_info(golden)["elem_bytes"] == 4
    want = check_frame(F, data, 15, 13, 4, True, "greedy")   # three blocks of 8 KB
    assert len(W4.blocks(want)) == 3
    check_frame(F, W4.figure_input("f32_sine"), 10, 13, 4, False, "lazy")
    # shuffle=0 is the frame there always was
    with open(os.path.join(O.GOLD, "laozi.txt.w15.b12.sqzf"), "rb") as fh:
        v1 = fh.read()
    assert sqz_amd.compress_frame(O.corpus("laozi.txt"), 15, 12, shuffle=0) == v1
    enc = F.FrameEncoder(len(O.corpus("laozi.txt")), 15, 12, shuffle=0)
    enc.encode(dev(O.corpus("laozi.txt")), len(O.corpus("laozi.txt")))
    assert enc.result() == v1


def test_noise_under_store_fits_the_bound_exactly(F):
    import sqz_amd
    data = W4.figure_input("u32_noise")
    want = check_frame(F, data, 15, 12, 4, True, "greedy")
    assert all(b["stored"] for b in W4.blocks(want))
    bound = F.frame_bound(len(data), 12, True, shuffle=4)
    assert len(want) == bound
    enc, frame, frame_bytes, status, err = encode_dev(F, data, 15, 12, 4, True, "greedy", capacity=bound - 8)
    assert status == E.E2BIG and frame_bytes == bound and (frame == GUARD).all()
    n, buf = C.c_uint64(0), (C.c_uint8 * bound)()
    from sqz_amd import _native as N
    assert N.lib().sqz_frame_compress_shuf(data, len(data), 15, 12, 5, 0, 4, buf, bound - 8, C.byref(n)) == E.E2BIG
    assert n.value == bound
    assert N.lib().sqz_frame_compress_shuf(data, len(data), 15, 12, 1, 0, 4, buf, bound, C.byref(n)) == 0
    assert bytes(buf[:n.value]) == want                      # SQZ_FRAME_SHUFFLE is set in the header either way


# ---------------------------------------------------------------- damage and refusals
@pytest.mark.parametrize("store", [False, True])
def test_a_flipped_payload_bit_is_eilseq_for_that_block_only(F, store):
    import sqz_amd
    data = content(2)
    frame = W4.write_frame(data, 15, 12, 2, store)
    blk = W4.blocks(frame)
    bad = bytearray(frame)
    bad[blk[2]["payload_off"] + 40] ^= 0x04
    out, errs = sqz_amd.decompress_frame(bytes(bad), return_errors=True)
    assert errs[2] != 0 and [errs[k] for k in (0, 1, 3, 4)] == [0, 0, 0, 0]
    assert out[:8192] == data[:8192] and out[12288:] == data[12288:]
    d_out = filled(len(data))
    derr, dstatus = F.decode_frame(dev(bad), d_out)
    sync()
    assert int(dstatus.item()) == 0 and host(derr).tolist()[2] != 0 and not host(derr)[[0, 1, 3, 4]].any()
    h = host(d_out).tobytes()
    assert h[:8192] == data[:8192] and h[12288:] == data[12288:]
    assert sqz_amd.read_range(bytes(bad), 100, 8000) == data[100:8100]     # a damaged block outside the range
    with pytest.raises(OSError):
        sqz_amd.read_range(bytes(bad), 8000, 400)
    if store:                                                # a stored block's content checksum notices as well
        noise = W4.figure_input("u32_noise")
        nf = bytearray(W4.write_frame(noise, 15, 12, 4, True))
        nf[W4.blocks(bytes(nf))[1]["payload_off"] + 7] ^= 0x80
        out, errs = sqz_amd.decompress_frame(bytes(nf), return_errors=True)
        assert errs == [0, E.EILSEQ, 0, 0, 0]


def test_a_wrong_record_is_refused_with_nothing_written(F):
    import sqz_amd
    data = content(4)
    frame = W4.write_frame(data, 15, 12, 4, True)
    info = sqz_amd.frame_info(frame)
    d_frame = dev(frame)
    for other in (2, 8):                                     # the caller's elem_bytes is not the record's
        d_out = filled(len(data))
        derr, dstatus = F.decode_frame(d_frame, d_out, info=dict(info, elem_bytes=other))
        part, rerr, rstatus = F.read_frame(d_frame, 4000, 200, d_out=filled(200), info=dict(info, elem_bytes=other))
        sync()
        assert int(dstatus.item()) == E.EINVAL and (host(derr) == E.EINVAL).all() and (host(d_out) == GUARD).all()
        assert int(rstatus.item()) == E.EINVAL and (host(part) == GUARD).all()
    plain = W4.write_frame(data, 15, 12, 4)
    for name, bad, _, want in W4.refusals(plain):
        d_out = filled(len(data))
        derr, dstatus = F.decode_frame(dev(bad), d_out, info=dict(sqz_amd.frame_info(plain)))
        sync()
        assert int(dstatus.item()) == want and (host(derr) == want).all() and (host(d_out) == GUARD).all(), name
        with pytest.raises(OSError) as ei:
            sqz_amd.decompress_frame(bad)
        assert ei.value.errno == want, name


def test_scratch_one_byte_smaller_is_einval_at_the_call(F):
    import torch
    from sqz_amd import _native as N
    L = N.lib()
    data = content(4)
    frame = W4.write_frame(data, 15, 12, 4, True)
    d_in, d_frame, d_out = dev(data), dev(frame), filled(len(data))
    cap = F.frame_bound(len(data), 12, True, shuffle=4)
    d_new, fb = filled(cap), torch.zeros(1, dtype=torch.int64, device="cuda")
    status, err = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    need = L.sqz_hip_frame_scratch_bytes_shuf(len(data), 12, 1, 5)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = (p(d_in), len(data), 15, 12, 5, 0, 4, p(d_new), cap, p(fb), p(status), p(err), p(scratch))
    assert L.sqz_hip_frame_encode_shuf(*args, need - 1, None) == E.EINVAL
    assert L.sqz_hip_frame_encode_shuf(*args, need, None) == 0
    sync()
    assert int(status.item()) == 0 and host(d_new)[:len(frame)].tobytes() == frame
    need = L.sqz_hip_frame_scratch_bytes_shuf(len(data), 12, 0, 4)
    args = (p(d_frame), len(frame), 5, len(data), 4, p(d_out), p(err), p(status), p(scratch))
    assert L.sqz_hip_frame_decode_shuf(*args, need - 1, None) == E.EINVAL
    sync()
    assert (host(d_out) == GUARD).all()
    assert L.sqz_hip_frame_decode_shuf(*args, need, None) == 0
    sync()
    assert int(status.item()) == 0 and host(d_out).tobytes() == data
    need = L.sqz_hip_frame_read_scratch_bytes_shuf(4097, 12)  # a range that starts at a block's last byte and ends with the next block
    part = filled(4097)
    args = (p(d_frame), len(frame), 5, len(data), 12, 4, 4095, 4097, p(part), p(err), p(status), p(scratch))
    assert L.sqz_hip_frame_read_shuf(*args, need - 1, None) == E.EINVAL
    assert L.sqz_hip_frame_read_shuf(*args, need, None) == 0
    sync()
    assert int(status.item()) == 0 and host(part).tobytes() == data[4095:8192]


# ---------------------------------------------------------------- ranged reads
@pytest.mark.parametrize("e", W4.ELEMS)
def test_ranged_reads(F, e):
    import sqz_amd
    data = content(e)
    frame = W4.write_frame(data, 15, 12, e, True)
    d_frame = dev(frame)
    m = 4096 // e
    ranges = [(m // 2, 10), (m - 3, 7), (3 * m + 1, m),      # inside a plane, across planes
              (4090, 12), (4095, 4098), (0, len(data)),      # across a block edge, three blocks, everything
              (16384, 5), (16386, 3), (16380, 9), (8192, 0), (len(data), 0)]       # the tail block
    for off, ln in ranges:
        assert sqz_amd.read_range(frame, off, ln) == data[off:off + ln], (off, ln)
        d_out = filled(ln + 16)
        part, rerr, rstatus = F.read_frame(d_frame, off, ln, d_out=d_out)
        sync()
        assert int(rstatus.item()) == 0 and not host(rerr).any(), (off, ln)
        assert host(d_out)[:ln].tobytes() == data[off:off + ln] and (host(d_out)[ln:] == GUARD).all(), (off, ln)
    with pytest.raises(OSError):
        sqz_amd.read_range(frame, len(data) - 1, 2)


# ---------------------------------------------------------------- the calls there were
def test_gather_update_append_and_the_old_readers_refuse_version_4(F):
    import sqz_amd
    data = content(4)
    for store in (False, True):
        frame = W4.write_frame(data, 15, 12, 4, store)
        d_frame = dev(frame)
        info = sqz_amd.frame_info(frame)
        for fn, args in ((F.gather_frame, ([0], [1])), (F.update_frame, ([0], [1], b"x")), (F.append_frame, (b"x",))):
            with pytest.raises(ValueError, match="version-4"):
                fn(d_frame, *args)
        # past the Python check, as a caller of the C ABI would come: the kernels refuse by arithmetic
        as_v2 = dict(info, version=2)
        d_out = filled(64)
        _, _, range_err, decoded, status = F.gather_frame(d_frame, [0, 5000], [8, 8], d_out=d_out, info=as_v2)
        sync()
        assert int(status.item()) == E.EINVAL and int(decoded.item()) == 0 and (host(d_out) == GUARD).all()
        d_new = filled(len(frame) + 4096)
        _, frame_bytes, _, _, encoded, status = F.update_frame(d_frame, [0], [1], b"x", d_out=d_new, info=as_v2)
        sync()
        assert int(status.item()) == E.EINVAL and (host(d_new) == GUARD).all()
        _, frame_bytes, encoded, status = F.append_frame(d_frame, b"more", d_out=d_new, info=as_v2)
        sync()
        assert int(status.item()) == E.EINVAL and (host(d_new) == GUARD).all()
        d_out = filled(len(data))
        derr, dstatus = F.decode_frame(d_frame, d_out, info=as_v2)           # sqz_hip_frame_decode
        part, rerr, rstatus = F.read_frame(d_frame, 10, 20, d_out=filled(20), info=as_v2)
        sync()
        assert int(dstatus.item()) == E.EINVAL and (host(d_out) == GUARD).all()
        assert int(rstatus.item()) == E.EINVAL and (host(part) == GUARD).all()
        with pytest.raises(OSError) as ei:
            sqz_amd.decompress_frame(frame, dictionary=b"abc")
        assert ei.value.errno == E.EINVAL
    # and the version-4 readers a frame of versions 1 and 2, which they take, and of version 3, which they do not
    from sqz_amd import _native as N
    text = O.corpus("laozi.txt")[:6000]
    out, n = (C.c_uint8 * 6000)(), C.c_uint64(0)
    for store in (False, True):
        old = sqz_amd.compress_frame(text, 12, 12, store=store)
        assert N.lib().sqz_frame_decompress_shuf(old, len(old), out, 6000, C.byref(n), None) == 0 and bytes(out) == text
        assert N.lib().sqz_frame_read_shuf(old, len(old), 4090, 12, out) == 0 and bytes(out[:12]) == text[4090:4102]
    v3 = sqz_amd.compress_frame(text, 12, 12, dictionary=text[:100])
    assert N.lib().sqz_frame_decompress_shuf(v3, len(v3), out, 6000, C.byref(n), None) == E.EINVAL
    assert N.lib().sqz_frame_read_shuf(v3, len(v3), 0, 1, out) == E.EINVAL
