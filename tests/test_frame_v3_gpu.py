"""GPU: SQZF version 3 in the device-resident flavour (FrameEncoder(dictionary=), decode_frame(dictionary=)) and
ranged reads from a resident frame (read_frame), against the independent writers tests/frame_writer*.py and the host
flavour.  The inputs are tests/frame_v3_cases.py: small contents whose layout corners (n = 0, the padding on even n,
a stored block between two streams, window 2^10 with D = 1023) and dictionary corners (dict_model.cases()) are
asserted from the writer before anything is compared; the writer's frames are computed once."""
import errno
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import frame_v3_cases as K
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = errno


@pytest.fixture(scope="module")
def F():
    import torch
    assert torch.cuda.is_available()
    import sqz_amd
    assert "gfx950" in sqz_amd.device_info()["name"]
    from sqz_amd import frame
    K.check_layout()
    return frame


def dev(b: bytes, slack: int = 64):
    import torch
    return torch.from_numpy(np.frombuffer(b + bytes(slack), np.uint8).copy()).cuda()


def filled(n: int):
    import torch
    return torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def mixed():
    """(dictionary, content, {store: the writer's frame}): three 4 KB blocks, the middle one noise"""
    dct, data = K.dct(), K.mixed()
    return dct, data, {store: K.frame(dct, data, 15, 12, store, False) for store in (False, True)}


# ---------------------------------------------------------------- the writer
@pytest.mark.parametrize("parse", ["greedy", "lazy"])
@pytest.mark.parametrize("store", [False, True])
def test_encoder_equals_the_writer_and_the_host_flavour(F, store, parse):
    import torch
    for name, wb, bb, dct, data in K.contents():
        want = K.frame(dct, data, wb, bb, store, parse == "lazy")
        enc = F.FrameEncoder(len(data), wb, bb, store=store, parse=parse, dictionary=dct)
        assert enc.capacity == F.frame_bound(len(data), bb, store, True) >= len(want), name
        enc.frame.fill_(0x5A)
        d_in = dev(data)
        frame, frame_bytes, status, err = enc.encode(d_in, len(data))
        torch.cuda.synchronize()
        what = (name, store, parse)
        assert int(status.item()) == 0 and not host(err).any(), what
        assert int(frame_bytes.item()) == len(want), what
        got = host(frame)[:len(want)].tobytes()
        assert got == want, (what, next(k for k in range(len(want)) if got[k] != want[k]))
        assert (host(frame)[len(want):] == 0x5A).all(), what
        assert got == F.compress_frame(data, wb, bb, store=store, parse=parse, dictionary=dct), what
        # ... and back, with the dictionary as a device tensor this time
        d_out = filled(len(data) + 32)
        derr, dstatus = F.decode_frame(frame, d_out, info=W3.fields(want), dictionary=dev(dct, 0))
        torch.cuda.synchronize()
        assert int(dstatus.item()) == 0 and not host(derr).any(), what
        assert host(d_out)[:len(data)].tobytes() == data and (host(d_out)[len(data):] == 0x5A).all(), what


def test_encoder_with_a_capacity_one_byte_short(F, mixed):
    import torch
    dct, data, want = mixed
    for store in (False, True):
        enc = F.FrameEncoder(len(data), 15, 12, capacity=len(want[store]) - 1, store=store, dictionary=dct)
        enc.frame.fill_(0x5A)
        frame, frame_bytes, status, err = enc.encode(dev(data), len(data))
        torch.cuda.synchronize()
        assert int(status.item()) == E.E2BIG and int(frame_bytes.item()) == len(want[store])
        assert (host(frame) == 0x5A).all()
        with pytest.raises(OSError) as e:
            enc.result()
        assert e.value.errno == E.E2BIG
    # the encoder is reusable, and a second content of another size takes the place of the first
    enc = F.FrameEncoder(len(data), 15, 12, store=True, dictionary=dct)
    for content in (data, data[:5000], data):
        enc.encode(dev(content), len(content))
        assert enc.result() == K.frame(dct, content, 15, 12, True, False)


# ---------------------------------------------------------------- the decoder with 1, 2, 4 and 8 waves
_WAVES_CHECK = r"""
import os, pickle, sys
sys.path.insert(0, os.environ["SQZ_ROOT"])
import numpy as np, torch
from sqz_amd import frame as F
with open(os.environ["SQZ_V3_CASE"], "rb") as fh:
    dct, data, frame, info = pickle.load(fh)
d_frame = torch.from_numpy(np.frombuffer(frame + bytes(64), np.uint8).copy()).cuda()
d_out = torch.full((len(data) + 32,), 0x5A, dtype=torch.uint8, device="cuda")
err, status = F.decode_frame(d_frame, d_out, info=info, dictionary=dct)
torch.cuda.synchronize()
assert int(status.item()) == 0 and not err.cpu().numpy().any(), (int(status.item()), err.cpu().numpy().tolist())
out = d_out.cpu().numpy()
assert out[:len(data)].tobytes() == data and (out[len(data):] == 0x5A).all()
got, err, status = F.read_frame(d_frame, 4000, 300, info=info, dictionary=dct)
torch.cuda.synchronize()
assert int(status.item()) == 0 and got.cpu().numpy().tobytes() == data[4000:4300]
print("waves ok", os.environ.get("SQZ_DECODE_WAVES"))
"""


@pytest.fixture(scope="module")
def waves_file(mixed, tmp_path_factory):
    dct, data, want = mixed
    p = tmp_path_factory.mktemp("frame_v3") / "case.pickle"
    with open(p, "wb") as fh:
        pickle.dump((dct, data, want[True], W3.fields(want[True])), fh)
    return str(p)


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_decoder_with_1_2_4_8_waves_per_stream(F, waves_file, waves):
    """SQZ_DECODE_WAVES is read once per process: every setting in a fresh child process of its own time limit"""
    env = dict(os.environ, SQZ_DECODE_WAVES=str(waves), SQZ_ROOT=ROOT, SQZ_V3_CASE=waves_file)
    p = subprocess.run([sys.executable, "-c", _WAVES_CHECK], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and f"waves ok {waves}" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---------------------------------------------------------------- refusals on the device
def decode(F, frame: bytes, data: bytes, dct, info=None):
    import torch
    d_out = filled(len(data) + 32)
    err, status = F.decode_frame(dev(frame), d_out, info=W3.fields(frame) if info is None else info, dictionary=dct)
    torch.cuda.synchronize()
    return int(status.item()), host(err).tolist(), host(d_out)


def test_decode_refuses_the_wrong_dictionary_and_the_wrong_frame(F, mixed):
    dct, data, want = mixed
    frame = want[True]
    for bad in (bytes([dct[0] ^ 1]) + dct[1:], dct[:-1], dct + b"x"):
        status, err, out = decode(F, frame, data, bad)
        assert status == E.EILSEQ and err == [E.EILSEQ] * 3 and (out == 0x5A).all()
    # frames of versions 1 and 2 through the version-3 call
    for plain in (W.write_frame(data, 15, 12), W2.write_frame(data, 15, 12)):
        status, err, out = decode(F, plain, data, dct, info=W2.fields(plain))
        assert status == E.EINVAL and err == [E.EINVAL] * 3 and (out == 0x5A).all()
    # a flipped byte of the record: index_crc notices before the record is compared
    for at in (32 + 24, 32 + 24 + 7):
        bad = bytearray(frame)
        bad[at] ^= 0x04
        status, err, out = decode(F, bytes(bad), data, dct)
        assert status == E.EILSEQ and err == [E.EILSEQ] * 3 and (out == 0x5A).all()
    # a flipped payload byte in block 2: that block's errno, blocks 0 and 1 delivered
    bad = bytearray(frame)
    bad[W3.blocks(frame)[2]["payload_off"] + 9] ^= 0x40
    status, err, out = decode(F, bytes(bad), data, dct)
    assert status == 0 and err[:2] == [0, 0] and err[2] != 0
    assert out[:8192].tobytes() == data[:8192] and (out[len(data):] == 0x5A).all()
    # ... and in the stored block 1, which no decoder reads: its checksum
    bad = bytearray(frame)
    bad[W3.blocks(frame)[1]["payload_off"] + 100] ^= 1
    status, err, out = decode(F, bytes(bad), data, dct)
    assert status == 0 and err == [0, E.EILSEQ, 0]
    # a frame cut short: the payload lies beyond avail
    import torch
    d_out = filled(len(data))
    err, status = F.decode_frame(dev(frame)[:len(frame) - 8], d_out, info=W3.fields(frame), dictionary=dct)
    torch.cuda.synchronize()
    assert int(status.item()) == E.E2BIG and (host(d_out) == 0x5A).all()


# ---------------------------------------------------------------- ranged reads
def _frames(mixed):
    dct, data, want = mixed
    v1, v2 = W.write_frame(data, 15, 12), W2.write_frame(data, 15, 12)
    assert W.fields(v1)["version"] == 1 and W2.fields(v2)["version"] == 2 and W3.fields(want[False])["version"] == 3
    return (("v1", v1, W.fields, None), ("v2", v2, W2.fields, None),
            ("v3", want[False], W3.fields, dct), ("v3_store", want[True], W3.fields, dct))


def read(F, d_frame, info, dct, at, n, room=None):
    import torch
    d_out = filled((n if room is None else room) + 32)
    got, err, status = F.read_frame(d_frame, at, n, d_out=d_out, info=info, dictionary=dct)
    torch.cuda.synchronize()
    assert got.numel() == n
    return int(status.item()), host(err).tolist(), host(d_out)


def test_read_frame_delivers_the_range_and_nothing_else(F, mixed):
    dct, data, want = mixed
    ranges = K.RANGES + ((0, len(data)), (len(data) - 1, 1), (4096, 4096), (0, 1))
    for name, frame, fields, d in _frames(mixed):
        d_frame, info = dev(frame), fields(frame)
        for at, n in ranges:
            status, err, out = read(F, d_frame, info, d, at, n)
            assert status == 0 and not any(err) and len(err) == ((at + n - 1) >> 12) - (at >> 12) + 1, (name, at, n)
            assert out[:n].tobytes() == data[at:at + n], (name, at, n)
            assert (out[n:] == 0x5A).all(), (name, at, n)
        # nothing to read: status 0, also where the content ends, and nothing written
        for at in (0, 5000, len(data)):
            status, err, out = read(F, d_frame, info, d, at, 0)
            assert status == 0 and err == [] and (out == 0x5A).all(), (name, at)
        # a range that leaves the content is refused at the call
        for at, n in ((len(data), 1), (8000, len(data) - 8000 + 1), (0, len(data) + 1), (len(data) + 1, 0)):
            with pytest.raises(OSError) as e:
                F.read_frame(d_frame, at, n, info=info, dictionary=d)
            assert e.value.errno == E.EINVAL, (name, at, n)
        # header fetched from the device when not given; d_out made when not given
        import torch
        got, err, status = F.read_frame(d_frame, 4090, 12, dictionary=d)
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and host(got).tobytes() == data[4090:4102]


def test_read_frame_and_damage(F, mixed):
    dct, data, want = mixed
    for name, frame, fields, d in _frames(mixed):
        info = fields(frame)
        bad = bytearray(frame)
        bad[len(frame) - 40] ^= 0x40                        # in block 2's stream, the last of the payload
        assert (W3 if name.startswith("v3") else W2).blocks(frame)[2]["payload_off"] < len(frame) - 40
        d_bad = dev(bytes(bad))
        # block 2 is covered: nothing is delivered; it is not: the range comes
        for at, n in ((8000, 400), (8500, 100), (0, len(data))):
            status, err, out = read(F, d_bad, info, d, at, n)
            assert status != 0 and err[-1] == status and not any(err[:-1]) and (out == 0x5A).all(), (name, at, n)
        for at, n in ((4090, 12), (0, 8192), (8191, 1)):
            status, err, out = read(F, d_bad, info, d, at, n)
            assert status == 0 and not any(err) and out[:n].tobytes() == data[at:at + n], (name, at, n)
    # the wrong dictionary, a version-3 frame without one, another frame with one, a caller whose block_bits is not
    # the frame's: the frame's status for every covering block, nothing delivered
    frame = want[True]
    for d, f, want_status in ((dct[:-1], frame, E.EILSEQ), (None, frame, E.EINVAL), (dct, W2.write_frame(data, 15, 12), E.EINVAL)):
        info = W3.fields(f) if f is frame else W2.fields(f)
        status, err, out = read(F, dev(f), info, d, 4090, 12)
        assert status == want_status and err == [want_status] * 2 and (out == 0x5A).all()
    one = K.frame(dct, data[:4096], 15, 12, False, False)
    info = dict(W3.fields(one), block_bytes=8192)
    status, err, out = read(F, dev(one), info, dct, 10, 20)
    assert status == E.EINVAL and err == [E.EINVAL] and (out == 0x5A).all()


def test_the_calls_on_a_stream_that_is_not_the_default(F, mixed):
    import torch
    dct, data, want = mixed
    frame = want[True]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        enc = F.FrameEncoder(len(data), 15, 12, store=True, dictionary=dct)
        d_frame, frame_bytes, status, err = enc.encode(dev(data), len(data))
        d_out = filled(len(data) + 32)
        derr, dstatus = F.decode_frame(d_frame, d_out, info=W3.fields(frame), dictionary=dct)
        part = filled(400 + 32)
        got, rerr, rstatus = F.read_frame(d_frame, 8000, 400, d_out=part, info=W3.fields(frame), dictionary=dct)
        plain = dev(W2.write_frame(data, 15, 12))
        part2 = filled(12 + 32)
        got2, rerr2, rstatus2 = F.read_frame(plain, 4090, 12, d_out=part2, info=W2.fields(W2.write_frame(data, 15, 12)))
    side.synchronize()
    assert int(status.item()) == 0 and host(d_frame)[:int(frame_bytes.item())].tobytes() == frame
    assert int(dstatus.item()) == 0 and not host(derr).any() and host(d_out)[:len(data)].tobytes() == data
    assert int(rstatus.item()) == 0 and host(part)[:400].tobytes() == data[8000:8400] and (host(part)[400:] == 0x5A).all()
    assert int(rstatus2.item()) == 0 and host(part2)[:12].tobytes() == data[4090:4102] and (host(part2)[12:] == 0x5A).all()
