"""GPU: batches with byte-shuffled (version 4) frames in them -- encode_frames(..., shuffle=[...]) and decode_frames(...,
shuffled=True) on the mixed batch of tests/frames_v4_cases.py against the independent writers (tests/frame_writer.py,
_v2.py, _v4.py), against the single calls (FrameEncoder, decode_frame) frame by frame, with fill bytes between and
behind everything a batch writes; the shuffle kernel for ranges of mixed element size against numpy; damage and
refusals that cost one block or one frame and nothing else; and compress_frames / decompress_frames."""
import errno
import functools
import os

import numpy as np
import pytest

import frame_gather_cases as G
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v4 as W4
import frames_v4_cases as V

pytestmark = pytest.mark.gpu
E = errno
FILL = 0xA5
WB, BITS, BB, K = V.WB, V.BITS, V.BB, V.K
GOLDEN_V4 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ramp_u32.w15.b12.e4.sqzf")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev(torch, data: bytes):
    return torch.from_numpy(np.frombuffer(bytes(data) + b"\0", np.uint8).copy())[:len(data)].cuda()


def encode_batch(torch, datas, elems, store, parse="greedy"):
    """encode_frames into a buffer of fill bytes -> (image, frame_at + [total], frame_bytes, err, status) on the host"""
    from sqz_amd import frame as F
    sizes = [len(d) for d in datas]
    total, frame_at = F.frames_bound(sizes, BITS, store, shuffle=elems)
    d_out = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
    got = F.encode_frames(dev(torch, b"".join(datas)), sizes, WB, BITS, store, parse, d_out=d_out, shuffle=elems)
    torch.cuda.synchronize()
    assert got[0] is d_out and got[1] == frame_at
    return d_out.cpu().numpy(), frame_at + [total], got[2].cpu().tolist(), got[3].cpu().tolist(), got[4].cpu().tolist()


@pytest.fixture(scope="module")
def batch(torch):
    made = {}

    def run(store):
        if store not in made:
            made[store] = encode_batch(torch, V.contents(), V.ELEMS, store)
        return made[store]
    return run


def single(torch, data, e, store):
    """(frame or b"", frame_bytes, status, err) of FrameEncoder for that content alone"""
    from sqz_amd import frame as F
    enc = F.FrameEncoder(max(len(data), 1), WB, BITS, store=store, shuffle=e)
    enc.encode(dev(torch, data), len(data))
    torch.cuda.synchronize()
    n = V.blocks_in(len(data))
    status, size = int(enc.status.item()), int(enc.frame_bytes.item())
    frame = enc.frame[:size].cpu().numpy().tobytes() if status == 0 else b""
    return frame, size, status, enc.err.cpu().tolist()[:n]


# ---------------------------------------------------------------------------------- the pass on its own
@pytest.mark.parametrize("inverse", [False, True])
def test_shuffle_ranges_on_the_blocks_of_the_mixed_batch_against_numpy(torch, inverse):
    from sqz_amd import _native as N
    from sqz_amd import frame as F
    blob = b"".join(V.contents())
    cuts, elems = [3], []                                    # the ranges: every block of the batch, 3 bytes into the buffers
    for f, data in enumerate(V.contents()):
        for b in W.blocks_of(data, BITS):
            cuts.append(cuts[-1] + len(b))
            elems.append(V.ELEMS[f])
    n = len(elems)
    skip = [1 if j % 7 == 3 else 0 for j in range(n)]
    src = np.frombuffer(bytes(3) + blob + bytes(16), np.uint8)
    d_src = dev(torch, src.tobytes())
    d_dst = torch.full((len(src) + 16,), FILL, dtype=torch.uint8, device="cuda")
    d_off = torch.tensor(cuts, dtype=torch.int64, device="cuda")
    d_elem = torch.tensor(elems, dtype=torch.int32, device="cuda")
    d_skip = torch.tensor(skip, dtype=torch.int32, device="cuda")
    rc = N.lib().sqz_hip_shuffle_ranges(F._ptr(d_src), F._ptr(d_off), F._ptr(d_elem), n, int(inverse), F._ptr(d_dst[1:]),
                                        F._ptr(d_skip), F._stream())
    torch.cuda.synchronize()
    assert rc == 0
    want = np.full(len(src) + 16, FILL, np.uint8)
    for a, b, e, s in zip(cuts, cuts[1:], elems, skip):
        if not s:
            blk = src[a:b].tobytes()
            out = blk if e == 0 else W4.unshuffle(blk, e) if inverse else W4.shuffle(blk, e)
            want[1 + a:1 + b] = np.frombuffer(out, np.uint8)
    assert (d_dst.cpu().numpy() == want).all()
    assert {0, 2, 4, 8} == set(elems) and n == sum(V.blocks_in(c) for c in V.LENGTHS)


# ---------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("store", [False, True])
def test_every_frame_of_the_mixed_batch_is_the_writers_and_the_single_calls(torch, batch, store):
    image, frame_at, frame_bytes, err, status = batch(store)
    assert status == [0] * K and not any(err) and len(err) == sum(V.blocks_in(c) for c in V.LENGTHS)
    for f, data in enumerate(V.contents()):
        want = V.frames(store)[f]
        got = image[frame_at[f]:frame_at[f] + frame_bytes[f]].tobytes()
        assert want[4] == (4 if V.ELEMS[f] else 2 if store else 1)
        assert frame_bytes[f] == len(want) and got == want, (f, len(data))
        one = single(torch, data, V.ELEMS[f], store)
        assert (got, frame_bytes[f], 0, [0] * V.blocks_in(len(data))) == one, (f, len(data))
        assert (image[frame_at[f] + frame_bytes[f]:frame_at[f + 1]] == FILL).all(), f    # between the frames
    assert (image[frame_at[-1]:] == FILL).all()                                            # and behind the last
    if store:
        assert all(b["stored"] for b in V.blocks(V.frames(True)[7]))                       # noise, in a version-4 frame


def test_one_element_size_for_every_frame_and_lazy_parse(torch):
    datas = [V.content(5), V.content(7), b"", V.content(3)]
    image, frame_at, frame_bytes, err, status = encode_batch(torch, datas, 4, True, "lazy")
    assert status == [0] * 4 and not any(err)
    for f, data in enumerate(datas):
        want = W4.write_frame(data, WB, BITS, 4, True, True)
        assert image[frame_at[f]:frame_at[f] + frame_bytes[f]].tobytes() == want, f


def test_all_element_sizes_zero_is_the_call_there_always_was(torch):
    from sqz_amd import frame as F
    for store in (False, True):
        sizes = V.LENGTHS
        total, frame_at = F.frames_bound(sizes, BITS, store)
        assert (total, frame_at) == F.frames_bound(sizes, BITS, store, shuffle=[0] * K)
        d_old = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
        old = F.encode_frames(dev(torch, b"".join(V.contents())), sizes, WB, BITS, store, d_out=d_old)
        torch.cuda.synchronize()
        new = encode_batch(torch, V.contents(), [0] * K, store)
        assert (d_old.cpu().numpy() == new[0]).all() and new[1] == frame_at + [total]
        assert [t.cpu().tolist() for t in old[2:]] == list(new[2:])
        assert new[4] == [0] * K


def test_the_time_stamps_in_the_middle_cost_what_the_single_call_says_and_their_frame_alone(torch):
    stamps = W4.figure_input("u64_stamps")
    frame, size, st, err = single(torch, stamps, 8, False)   # today: E2BIG from the emit kernel's tree guard, nothing written
    datas = [V.content(5), stamps, V.content(6)]
    elems = [4, 8, 2]
    image, frame_at, frame_bytes, berr, status = encode_batch(torch, datas, elems, False)
    n0 = V.blocks_in(len(datas[0]))
    n1 = V.blocks_in(len(stamps))
    assert status == [0, st, 0] and berr[n0:n0 + n1] == err and not any(berr[:n0]) and not any(berr[n0 + n1:])
    assert frame_bytes[1] == size
    if st == 0:
        assert image[frame_at[1]:frame_at[1] + size].tobytes() == frame
    else:
        assert (image[frame_at[1]:frame_at[2]] == FILL).all()
    for f in (0, 2):
        want = W4.write_frame(datas[f], WB, BITS, elems[f])
        assert image[frame_at[f]:frame_at[f] + frame_bytes[f]].tobytes() == want
        assert (image[frame_at[f] + frame_bytes[f]:frame_at[f + 1]] == FILL).all()


# ---------------------------------------------------------------------------------- decode
@functools.lru_cache(maxsize=None)
def decode_set(store):
    """[(frame, content)]: the mixed batch, the golden version-4 frame and a version-2 frame of 8 KB blocks at 2^12"""
    out = list(zip(V.frames(store), V.contents()))
    with open(GOLDEN_V4, "rb") as fh:
        out.insert(4, (fh.read(), W4.figure_input("u32_ramp")))
    other = G.content("whole") + G.piece("N")[:1000] + G.piece("b")[:333]
    out.insert(7, (W2.write_frame(other, 12, 13), other))
    return out


def lay(torch, frames, gap=16):
    """the frames at multiples of 16, `gap` fill bytes and more between them -> (device image, frame_at)"""
    frame_at, at = [], 0
    for fr in frames:
        frame_at.append(at)
        at += V.pad16(len(fr)) + gap
    image = np.full(at + 16, FILL, np.uint8)
    for a, fr in zip(frame_at, frames):
        image[a:a + len(fr)] = np.frombuffer(fr, np.uint8)
    return torch.from_numpy(image).cuda(), frame_at


def decode(torch, frames, sizes, infos=None, shuffled=True):
    """decode_frames into fill bytes with gaps of 5, 10, ... between the outputs -> (image, out_at, err, status)"""
    from sqz_amd import frame as F
    d_frames, frame_at = lay(torch, frames)
    out_at, at = [], 7
    for f, c in enumerate(sizes):
        out_at.append(at)
        at += c + 5 * (f + 1)
    d_out = torch.full((at + 32,), FILL, dtype=torch.uint8, device="cuda")
    got = F.decode_frames(d_frames, frame_at, infos, d_out, out_at, shuffled=shuffled)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_at, got[2].cpu().tolist(), got[3].cpu().tolist()


def check_outputs(image, out_at, contents, delivered):
    """delivered[f]: True, False (nothing written) or a set of blocks that are not"""
    want = np.full(len(image), FILL, np.uint8)
    for f, data in enumerate(contents):
        if delivered[f] is True:
            want[out_at[f]:out_at[f] + len(data)] = np.frombuffer(data, np.uint8)
    loose = np.ones(len(image), bool)                        # a block that failed: whatever the decoder left there
    for f, data in enumerate(contents):
        if isinstance(delivered[f], tuple):
            bb, bad = delivered[f]
            for b in range((len(data) + bb - 1) // bb):
                lo, hi = out_at[f] + b * bb, out_at[f] + min((b + 1) * bb, len(data))
                if b in bad:
                    loose[lo:hi] = False
                else:
                    want[lo:hi] = np.frombuffer(data[b * bb:(b + 1) * bb], np.uint8)
    assert (image[loose] == want[loose]).all()


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("with_infos", [False, True])
def test_a_mixed_batch_of_versions_1_2_and_4_decodes_with_the_gaps_untouched(torch, store, with_infos):
    from sqz_amd import frame as F
    frames, contents = zip(*decode_set(store))
    infos = [F.frame_info(fr) for fr in frames] if with_infos else None
    assert {fr[4] for fr in frames} == ({2, 4} if store else {1, 2, 4})
    image, out_at, err, status = decode(torch, frames, [len(c) for c in contents], infos)
    assert status == [0] * len(frames) and not any(err)
    check_outputs(image, out_at, contents, [True] * len(frames))


def test_without_shuffled_a_version_4_frame_is_still_einval_alone(torch):
    frames, contents = zip(*decode_set(False))
    image, out_at, err, status = decode(torch, frames, [len(c) for c in contents], shuffled=False)
    want = [E.EINVAL if fr[4] == 4 else 0 for fr in frames]
    assert status == want and 0 < sum(1 for s in want if s) < len(want)
    check_outputs(image, out_at, contents, [s == 0 for s in want])


def test_a_flipped_payload_byte_costs_one_block_of_one_frame(torch):
    from sqz_amd import frame as F
    noise = W4.figure_input("u32_noise")
    for stored in (True, False):
        frames, contents = map(list, zip(*decode_set(True)))
        if stored:                                           # five stored blocks in a version-4 frame: only the checksum
            frames.insert(2, W4.write_frame(noise, WB, BITS, 4, True))     # can notice, so the errno is EILSEQ exactly
            contents.insert(2, noise)
            f = 2
            assert all(b["stored"] for b in W4.blocks(frames[f]))
        else:                                                # a stream: whatever the single call says about that block
            f = next(j for j, fr in enumerate(frames) if fr[4] == 4 and W.fields(fr)["n_blocks"] >= 4)
            assert not W4.blocks(frames[f])[2]["stored"]
        blk = W4.blocks(frames[f])
        bad = bytearray(frames[f])
        bad[blk[2]["payload_off"] + blk[2]["payload_bytes"] // 2] ^= 0x40
        frames[f] = bytes(bad)
        d_frame = dev(torch, frames[f] + bytes(-len(frames[f]) % 16))[:len(frames[f])]
        d_back = torch.zeros(len(contents[f]), dtype=torch.uint8, device="cuda")
        derr, dstatus = F.decode_frame(d_frame, d_back)
        torch.cuda.synchronize()
        one = derr.cpu().tolist()
        assert int(dstatus.item()) == 0 and one[2] != 0 and [k for k, e in enumerate(one) if e] == [2]
        image, out_at, err, status = decode(torch, frames, [len(c) for c in contents])
        g0 = sum(W.fields(fr)["n_blocks"] for fr in frames[:f])
        assert status == [0] * len(frames)
        assert err[g0 + 2] == one[2] and not any(err[:g0 + 2]) and not any(err[g0 + 3:])
        if stored:
            assert err[g0 + 2] == E.EILSEQ
        check_outputs(image, out_at, contents, [True if j != f else (BB, {2}) for j in range(len(frames))])


def test_refusals_in_the_middle_cost_their_frame_alone(torch):
    from sqz_amd import frame as F
    base, contents = map(list, zip(*decode_set(True)))
    v3 = G.frame("mixed", 3)
    f4 = next(j for j, fr in enumerate(base) if fr[4] == 4 and W.fields(fr)["n_blocks"] >= 2)
    f2 = next(j for j, fr in enumerate(base) if fr[4] == 2 and W.fields(fr)["n_blocks"] >= 2)
    # a version-3 frame in the middle
    frames, datas = list(base), list(contents)
    frames.insert(3, v3)
    datas.insert(3, G.content("mixed"))
    image, out_at, err, status = decode(torch, frames, [len(c) for c in datas])
    assert status == [E.EINVAL if j == 3 else 0 for j in range(len(frames))]
    check_outputs(image, out_at, datas, [j != 3 for j in range(len(frames))])
    # the caller's element size is not the record's; one named for a version-2 frame; none for a version-4 frame
    for f, elem in ((f4, 2 if F.frame_info(base[f4])["elem_bytes"] != 2 else 4), (f2, 4), (f4, 0)):
        infos = [dict(F.frame_info(fr)) for fr in base]
        infos[f]["version"], infos[f]["elem_bytes"] = 4, elem
        image, out_at, err, status = decode(torch, base, [len(c) for c in contents], infos)
        assert status == [E.EINVAL if j == f else 0 for j in range(len(base))], (f, elem)
        g0 = sum(W.fields(fr)["n_blocks"] for fr in base[:f])
        n = W.fields(base[f])["n_blocks"]
        assert err[g0:g0 + n] == [E.EINVAL] * n and not any(err[:g0]) and not any(err[g0 + n:])
        check_outputs(image, out_at, contents, [j != f for j in range(len(base))])


def test_the_batch_decodes_what_the_single_call_decodes(torch):
    from sqz_amd import frame as F
    frames, contents = zip(*decode_set(True))
    image, out_at, err, status = decode(torch, frames, [len(c) for c in contents])
    b0 = 0
    for f, (fr, data) in enumerate(zip(frames, contents)):
        d_frame = dev(torch, fr + bytes(-len(fr) % 16))[:len(fr)]
        d_back = torch.full((max(len(data), 1),), FILL, dtype=torch.uint8, device="cuda")
        derr, dstatus = F.decode_frame(d_frame, d_back)
        torch.cuda.synchronize()
        n = W.fields(fr)["n_blocks"]
        assert int(dstatus.item()) == status[f] == 0 and derr.cpu().tolist() == err[b0:b0 + n]
        assert d_back.cpu().numpy()[:len(data)].tobytes() == data == image[out_at[f]:out_at[f] + len(data)].tobytes()
        b0 += n


# ---------------------------------------------------------------------------------- the host conveniences
@pytest.mark.parametrize("store", [False, True])
def test_compress_frames_and_decompress_frames_round_trip(torch, store):
    import sqz_amd
    frames = sqz_amd.compress_frames(V.contents(), WB, BITS, store, shuffle=V.ELEMS)
    assert frames == V.frames(store)
    assert sqz_amd.decompress_frames(frames, shuffled=True) == V.contents()
    assert sqz_amd.compress_frames(V.contents()[3:6], WB, BITS, store, shuffle=8) == \
        [W4.write_frame(d, WB, BITS, 8, store) for d in V.contents()[3:6]]
    with pytest.raises(sqz_amd.SqzError) as info:            # the default still refuses version 4
        sqz_amd.decompress_frames(frames)
    assert info.value.errno == E.EINVAL and info.value.frame == 0
    contents, errors = sqz_amd.decompress_frames(frames, return_errors=True)
    assert [s for s, _ in errors] == [E.EINVAL if e else 0 for e in V.ELEMS]
    assert contents == [b"" if e else c for e, c in zip(V.ELEMS, V.contents())]
