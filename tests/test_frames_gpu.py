"""GPU: encode_frames / decode_frames -- many SQZF frames in one call -- against the independent writers
(tests/frame_writer.py, frame_writer_v2.py), against the single calls (FrameEncoder, decode_frame) frame by frame, with
guard bytes between and behind everything a batch writes; damage that costs one block or one frame and nothing else;
and the host conveniences compress_frames / decompress_frames."""
import errno
import functools
import os

import numpy as np
import pytest

import frame_gather_cases as G
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v4 as W4
import oracle_lib as O

pytestmark = pytest.mark.gpu
E = errno
FILL = 0xA5
BB, BITS, WB = G.BB, G.BITS, G.WB
GOLDEN_V4 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ramp_u32.w15.b12.e4.sqzf")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev(torch, data: bytes):
    return torch.from_numpy(np.frombuffer(bytes(data) + b"\0", np.uint8).copy())[:len(data)].cuda()


@functools.lru_cache(maxsize=None)
def contents():
    """0, 1, 4096, 4097, 3 * 4096 + 5, 70 * 4096 and 300 * 4096 - 1 bytes, and noise so that stored blocks occur"""
    out = (b"", b"q", G.piece("A"), G.piece("b") + b"z", G.piece("a") + G.piece("A") + G.piece("c") + b"hello",
           G.content("b70")[:69 * BB] + G.piece("p"), G.content("b300")[:299 * BB] + G.piece("k")[:BB - 1],
           W2.random_bytes(2 * BB + 77, 5))
    assert [len(c) for c in out[:7]] == [0, 1, 4096, 4097, 3 * 4096 + 5, 70 * 4096, 300 * 4096 - 1]
    return out


MOST = 300 * BB


@functools.lru_cache(maxsize=None)
def stream_of(block: bytes, lazy: bool) -> bytes:
    return W4.stream_of(block, WB, lazy)


@functools.lru_cache(maxsize=None)
def writers_frame(f: int, lazy: bool, store: bool) -> bytes:
    data = contents()[f]
    streams = [stream_of(b, lazy) for b in W.blocks_of(data, BITS)]
    return (W2.assemble if store else W.assemble)(data, WB, BITS, streams)


@pytest.fixture(scope="module")
def batch(torch):
    """batch(parse, store) -> what encode_frames left for all contents, on the host, each combination once"""
    from sqz_amd import frame as F
    made = {}

    def run(parse, store):
        if (parse, store) not in made:
            sizes = [len(c) for c in contents()]
            total, frame_at = F.frames_bound(sizes, BITS, store)
            d_out = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
            got = F.encode_frames(dev(torch, b"".join(contents())), sizes, WB, BITS, store, parse, d_out=d_out)
            torch.cuda.synchronize()
            assert got[0] is d_out and got[1] == frame_at
            made[(parse, store)] = (d_out.cpu().numpy(), frame_at + [total], got[2].cpu().tolist(), got[3].cpu().tolist(),
                                    got[4].cpu().tolist())
        return made[(parse, store)]
    return run


@pytest.fixture(scope="module")
def single(torch):
    """single(parse, store, content) -> (frame, frame_bytes, status, err) of FrameEncoder for that content alone"""
    from sqz_amd import frame as F
    encoders = {}

    def run(parse, store, data):
        if (parse, store) not in encoders:
            encoders[(parse, store)] = F.FrameEncoder(MOST, WB, BITS, store=store, parse=parse)
        enc = encoders[(parse, store)]
        enc.encode(dev(torch, data))
        frame = enc.result()
        n = (len(data) + BB - 1) >> BITS
        return frame, int(enc.frame_bytes.item()), int(enc.status.item()), enc.err.cpu().tolist()[:n]
    return run


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("parse", ["greedy", "lazy"])
def test_every_frame_of_a_batch_is_the_writers_and_the_single_calls(torch, batch, single, parse, store):
    image, frame_at, frame_bytes, err, status = batch(parse, store)
    assert status == [0] * len(contents()) and not any(err)
    assert len(err) == sum((len(c) + BB - 1) >> BITS for c in contents())
    for f, data in enumerate(contents()):
        want = writers_frame(f, parse == "lazy", store)
        got = image[frame_at[f]:frame_at[f] + frame_bytes[f]].tobytes()
        assert frame_bytes[f] == len(want) and got == want, (f, len(data))
        assert got == single(parse, store, data)[0], (f, len(data))
        assert (image[frame_at[f] + frame_bytes[f]:frame_at[f + 1]] == FILL).all(), f    # between the frames
    assert (image[frame_at[-1]:] == FILL).all()                                            # and behind the last
    if store:
        stored = [b["stored"] for b in W2.blocks(writers_frame(7, parse == "lazy", True))]
        assert any(stored)


@pytest.mark.parametrize("store", [False, True])
def test_a_batch_of_one_is_the_single_call(torch, single, store):
    from sqz_amd import frame as F
    data = contents()[4]
    _, _, frame_bytes, err, status = F.encode_frames(dev(torch, data), [len(data)], WB, BITS, store)
    torch.cuda.synchronize()
    _, want_bytes, want_status, want_err = single("greedy", store, data)
    assert frame_bytes.cpu().tolist() == [want_bytes] and status.cpu().tolist() == [want_status] == [0]
    assert err.cpu().tolist() == want_err


@functools.lru_cache(maxsize=None)
def other_frames():
    """frames of another window and 8 KB blocks, one of either version, from the writers"""
    data = G.content("whole") + G.piece("N")[:1000] + G.piece("b")[:333]
    return ((data, W.write_frame(data, 12, 13)), (data, W2.write_frame(data, 12, 13)))


@pytest.fixture(scope="module")
def resident(torch, batch):
    """the frames of a decode: the batch's own of either version (writers_frame's bytes: tested above) and the writers'
    with other parameters, laid out 16-byte aligned with a gap behind every other one -> (device image, frame_at,
    contents, host frames)"""
    frames = [(contents()[f], writers_frame(f, False, f % 2 == 1)) for f in range(len(contents()))]
    frames[3:3] = list(other_frames())
    frames.append((contents()[5], writers_frame(5, True, True)))
    at, frame_at = 0, []
    for j, (_, fr) in enumerate(frames):
        frame_at.append(at)
        at += ((len(fr) + 15) & ~15) + 16 * (j % 2)
    image = np.full(at + 16, FILL, np.uint8)
    for a, (_, fr) in zip(frame_at, frames):
        image[a:a + len(fr)] = np.frombuffer(fr, np.uint8)
    return torch.from_numpy(image).cuda(), frame_at, [d for d, _ in frames], [fr for _, fr in frames], image


def block_base(frames):
    return np.cumsum([0] + [W.fields(fr)["n_blocks"] for fr in frames]).tolist()


def test_decode_of_a_mixed_batch_packed_and_with_gaps(torch, resident):
    from sqz_amd import frame as F
    d_frames, frame_at, datas, frames, _ = resident
    assert {W.fields(fr)["version"] for fr in frames} == {1, 2} and {W.fields(fr)["block_bytes"] for fr in frames} == {BB, 2 * BB}
    d_out, out_at, err, status = F.decode_frames(d_frames, frame_at)
    torch.cuda.synchronize()
    assert out_at == np.cumsum([0] + [len(d) for d in datas])[:-1].tolist()
    assert status.cpu().tolist() == [0] * len(frames) and not err.cpu().numpy().any()
    assert err.numel() == block_base(frames)[-1]
    assert d_out.cpu().numpy().tobytes() == b"".join(datas)
    # gaps between the outputs and a tail behind them, infos given: all untouched
    out_at, at = [], 7
    for j, d in enumerate(datas):
        out_at.append(at)
        at += len(d) + 3 * (j % 4)
    room = torch.full((at + 50,), FILL, dtype=torch.uint8, device="cuda")
    infos = [F.frame_info(fr[:32]) for fr in frames]
    got, got_at, err, status = F.decode_frames(d_frames, frame_at, infos=infos, d_out=room, out_at=out_at)
    torch.cuda.synchronize()
    assert got is room and got_at == out_at and status.cpu().tolist() == [0] * len(frames) and not err.cpu().numpy().any()
    want = np.full(at + 50, FILL, np.uint8)
    for o, d in zip(out_at, datas):
        want[o:o + len(d)] = np.frombuffer(d, np.uint8)
    assert (room.cpu().numpy() == want).all()


def decode_damaged(torch, resident, change, infos_given=True):
    """a decode of the resident frames with `change(image)` applied -> (output over FILL, err, status, out_at)"""
    from sqz_amd import frame as F
    _, frame_at, datas, frames, image = resident
    image = image.copy()
    change(image)
    infos = [F.frame_info(fr[:32]) for fr in frames] if infos_given else None
    room = torch.full((sum(len(d) for d in datas) + 40,), FILL, dtype=torch.uint8, device="cuda")
    d_frames = torch.from_numpy(image).cuda()
    _, out_at, err, status = F.decode_frames(d_frames, frame_at, infos=infos, d_out=room)
    torch.cuda.synchronize()
    return room.cpu().numpy(), err.cpu().tolist(), status.cpu().tolist(), out_at, d_frames


def test_a_flipped_payload_byte_costs_its_block_alone(torch, resident):
    from sqz_amd import frame as F
    _, frame_at, datas, frames, _ = resident
    base = block_base(frames)
    f = 7                                                    # the 70-block frame of version 2, in the middle
    blk = W2.blocks(frames[f])
    assert W.fields(frames[f])["version"] == 2 and len(blk) == 70
    stored = next(b for b in range(20, 70) if blk[b]["stored"])
    stream = next(b for b in range(20, 70) if not blk[b]["stored"])
    for b, exact in ((stored, True), (stream, False)):
        spot = frame_at[f] + blk[b]["payload_off"] + blk[b]["payload_bytes"] // 2

        def flip(image):
            image[spot] ^= 0x40
        out, err, status, out_at, d_frames = decode_damaged(torch, resident, flip)
        assert status == [0] * len(frames)
        bad = base[f] + b
        assert err[bad] != 0 and [k for k, e in enumerate(err) if e != 0] == [bad]
        if exact:
            assert err[bad] == E.EILSEQ                      # a stored block: only the checksum can notice
        # what the single call leaves for that frame
        one = torch.full((len(datas[f]),), FILL, dtype=torch.uint8, device="cuda")
        one_err, one_status = F.decode_frame(d_frames[frame_at[f]:frame_at[f] + len(frames[f])], one)
        torch.cuda.synchronize()
        assert one_status.item() == 0 and one_err.cpu().tolist() == err[base[f]:base[f + 1]]
        want = np.frombuffer(b"".join(datas), np.uint8)
        lo, hi = out_at[f] + b * BB, out_at[f] + min((b + 1) * BB, len(datas[f]))
        keep = np.ones(len(want), bool)
        keep[lo:hi] = False                                  # the failed block holds whatever the decoder produced
        assert (out[:len(want)][keep] == want[keep]).all() and (out[len(want):] == FILL).all()


def test_a_flipped_header_byte_costs_its_frame_alone(torch, resident):
    _, frame_at, datas, frames, _ = resident
    base = block_base(frames)
    want = np.frombuffer(b"".join(datas), np.uint8)
    for f, at, infos_given, code in ((7, 28, True, E.EILSEQ), (4, 9, True, E.EINVAL), (7, 0, False, E.EINVAL)):
        def flip(image):
            image[frame_at[f] + at] ^= 0x01
        out, err, status, out_at, _ = decode_damaged(torch, resident, flip, infos_given)
        assert status == [code if j == f else 0 for j in range(len(frames))]
        if infos_given:
            assert err == [code if base[f] <= k < base[f + 1] else 0 for k in range(base[-1])]
            keep = np.ones(len(want), bool)
            keep[out_at[f]:out_at[f] + len(datas[f])] = False
            assert (out[:len(want)][keep] == want[keep]).all()
            assert (out[:len(want)][~keep] == FILL).all() and (out[len(want):] == FILL).all()
        else:                                                # a header that does not parse: a frame of no blocks there
            assert not any(err) and len(err) == base[-1] - (base[f + 1] - base[f])
            rest = b"".join(d for j, d in enumerate(datas) if j != f)
            assert out[:len(rest)].tobytes() == rest and (out[len(rest):] == FILL).all()


def test_a_version_4_frame_in_a_batch_is_einval_alone(torch, resident):
    from sqz_amd import frame as F
    with open(GOLDEN_V4, "rb") as fh:
        v4 = fh.read()
    info4 = F.frame_info(v4)
    assert info4["version"] == 4 and info4["n_blocks"] > 0
    frames = [writers_frame(4, False, True), v4, writers_frame(3, False, False)]
    datas = [contents()[4], bytes(info4["content_bytes"]), contents()[3]]
    at, frame_at = 0, []
    for fr in frames:
        frame_at.append(at)
        at += (len(fr) + 15) & ~15
    image = np.zeros(at, np.uint8)
    for a, fr in zip(frame_at, frames):
        image[a:a + len(fr)] = np.frombuffer(fr, np.uint8)
    room = torch.full((sum(len(d) for d in datas),), FILL, dtype=torch.uint8, device="cuda")
    _, out_at, err, status = F.decode_frames(torch.from_numpy(image).cuda(), frame_at, d_out=room)
    torch.cuda.synchronize()
    n = [(len(d) + BB - 1) >> BITS for d in datas]
    assert status.cpu().tolist() == [0, E.EINVAL, 0]
    assert err.cpu().tolist() == [0] * n[0] + [E.EINVAL] * n[1] + [0] * n[2]
    out = room.cpu().numpy()
    assert out[:len(datas[0])].tobytes() == datas[0] and out[out_at[2]:].tobytes() == datas[2]
    assert (out[out_at[1]:out_at[2]] == FILL).all()


def test_round_trips_through_the_host_conveniences(torch):
    from sqz_amd import frame as F
    from sqz_amd.codec import SqzError
    lao = O.corpus("laozi.txt")
    datas = [b"", lao[:1], lao[:3 * BB + 100], b"", lao[5000:5000 + BB], lao]
    for store in (False, True):
        frames = F.compress_frames(datas, WB, BITS, store=store)
        assert frames == [F.compress_frame(d, WB, BITS, store=store) for d in datas]
        assert F.decompress_frames(frames) == datas
    assert F.compress_frames([]) == [] and F.decompress_frames([]) == []
    mixed = F.compress_frames(datas, 12, 13, parse="lazy") + frames
    assert F.decompress_frames(mixed) == datas + datas
    bad = bytearray(frames[2])
    last = F.frame_blocks(frames[2])[3]
    bad[last["payload_off"] + last["payload_bytes"] // 2] ^= 0x10      # in the middle of the last block's share
    broken = frames[:2] + [bytes(bad)] + frames[3:]
    with pytest.raises(SqzError, match="frame 2") as caught:
        F.decompress_frames(broken)
    assert caught.value.frame == 2 and caught.value.block_errors[:3] == [0, 0, 0] and caught.value.block_errors[3] != 0
    got, errors = F.decompress_frames(broken, return_errors=True)
    assert [g for j, g in enumerate(got) if j != 2] == [d for j, d in enumerate(datas) if j != 2]
    assert got[2][:3 * BB] == datas[2][:3 * BB]
    assert [st for st, _ in errors] == [0] * len(datas) and [any(b) for _, b in errors] == [j == 2 for j in range(len(datas))]
