"""GPU: gather_frame -- many byte ranges of a device-resident frame in one call -- on frames written by FrameEncoder,
against the plain content (the model and the range lists of tests/frame_gather_cases.py)."""
import errno

import numpy as np
import pytest

import frame_gather_cases as G

pytestmark = pytest.mark.gpu
E = errno
FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def frames(torch):
    """{(name, version, parse): (device frame, info)}, each encoded once"""
    from sqz_amd import frame as F
    made = {}

    def get(name, version, parse="greedy"):
        key = (name, version, parse)
        if key not in made:
            data = G.content(name)
            enc = F.FrameEncoder(len(data), G.WB, G.BITS, store=version >= 2, parse=parse,
                                 dictionary=G.dct() if version == 3 else None)
            enc.encode(torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda())
            host = enc.result()
            info = F.frame_info(host)
            assert info["version"] == version and info["n_blocks"] == len(G.PATTERNS[name])
            made[key] = (enc.frame[:len(host)].clone(), info, host)
        return made[key]
    return get


def gather(torch, frame, info, offsets, lengths, cap, version, dictionary="default", **kw):
    from sqz_amd import frame as F
    if dictionary == "default":
        dictionary = G.dct() if version == 3 else None
    if "d_out" not in kw:
        total = G.model(b"\0" * info["content_bytes"], offsets, lengths, cap)[1][-1] if not torch.is_tensor(offsets) else kw.pop("total")
        kw["d_out"] = torch.full((total + 32,), FILL, dtype=torch.uint8, device="cuda")
    out, out_off, rerr, dec, st = F.gather_frame(frame, offsets, lengths, max_length=cap, info=info, dictionary=dictionary, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_off.cpu().tolist(), rerr.cpu().tolist(), int(dec.item()), int(st.item())


def check(got, data, offsets, lengths, cap, what, bad_blocks=(), bad_errno=E.EILSEQ):
    out, out_off, rerr, dec, st = got
    parts, want_off, want_err, blocks = G.model(data, offsets, lengths, cap, bad_blocks, bad_errno)
    assert (st, dec) == (0, len(blocks)), what
    assert out_off == want_off and rerr == want_err, what
    for r, p in enumerate(parts):
        piece = out[want_off[r]:want_off[r + 1]]
        assert (piece == FILL).all() if p is None else piece.tobytes() == p, (what, r)
    assert (out[want_off[-1]:] == FILL).all(), what


def _device_lists(torch, offsets, lengths, cap):
    """the invalid lists do not pass gather_frame's host check: they go up as tensors, as a kernel's would"""
    signed = lambda vs: torch.tensor([v - (1 << 64) if v >> 63 else v for v in vs], dtype=torch.int64, device="cuda")
    return signed(offsets), signed(lengths)


@pytest.mark.parametrize("version,name,parse", [(1, "mixed", "greedy"), (2, "mixed", "greedy"), (3, "mixed", "greedy"),
                                                (3, "mixed", "lazy"), (2, "whole", "greedy"), (3, "short", "greedy"),
                                                (1, "b70", "greedy"), (3, "b70", "greedy"), (2, "b300", "greedy"),
                                                (3, "b300", "greedy")])
def test_every_list_against_the_content(torch, frames, version, name, parse):
    frame, info, _ = frames(name, version, parse)
    data = G.content(name)
    for key, (offsets, lengths, cap) in G.range_lists(name).items():
        total = G.model(data, offsets, lengths, cap)[1][-1]
        if key == "invalid":
            o, ln = _device_lists(torch, offsets, lengths, cap)
            got = gather(torch, frame, info, o, ln, cap, version, total=total)
        else:
            got = gather(torch, frame, info, offsets, lengths, cap, version)
        check(got, data, offsets, lengths, cap, (version, name, key))


def test_one_range_equals_read_frame_and_the_dictionary_may_be_a_tensor(torch, frames):
    from sqz_amd import frame as F
    frame, info, _ = frames("mixed", 3)
    data = G.content("mixed")
    d_dict = torch.from_numpy(np.frombuffer(G.dct(), np.uint8).copy()).cuda()
    for at, n in ((4090, 12), (8000, 400), (0, len(data))):
        part, _, rst = F.read_frame(frame, at, n, info=info, dictionary=G.dct())
        got = gather(torch, frame, info, [at], [n], n, 3, dictionary=d_dict)
        torch.cuda.synchronize()
        assert int(rst.item()) == 0 and got[0][:n].tobytes() == part.cpu().numpy().tobytes() == data[at:at + n]
        check(got, data, [at], [n], n, (at, n))


def test_offsets_computed_on_the_device(torch, frames):
    frame, info, _ = frames("b300", 3)
    data = G.content("b300")
    count, n = 1000, 96
    offsets = (torch.arange(count, device="cuda", dtype=torch.int64) * 7919 * 131) % (len(data) - n)
    lengths = torch.full((count,), n, dtype=torch.int64, device="cuda")
    got = gather(torch, frame, info, offsets, lengths, n, 3, total=count * n)      # nothing went through the host
    host = [(k * 7919 * 131) % (len(data) - n) for k in range(count)]
    check(got, data, host, [n] * count, n, "device offsets")


def test_the_three_statuses_and_a_launch_wider_than_the_count(torch, frames):
    frame, info, _ = frames("b70", 2)
    data = G.content("b70")
    offsets, lengths, cap = G.range_lists("b70")["word_edges"]
    parts, want_off, want_err, blocks = G.model(data, offsets, lengths, cap)
    count, total = len(blocks), want_off[-1]
    check(gather(torch, frame, info, offsets, lengths, cap, 2, max_blocks=count), data, offsets, lengths, cap, "exact")
    # max_blocks = n_blocks with three blocks covered: the decode launch is wider than the count
    o3, l3, c3 = G.range_lists("b70")["two_edges"]
    got = gather(torch, frame, info, o3, l3, c3, 2, max_blocks=70)
    assert got[3] == 3
    check(got, data, o3, l3, c3, "wide launch")
    for m, room, want in ((count - 1, total, E.ENOBUFS), (count, total - 1, E.ENOSPC), (count - 1, total - 1, E.ENOBUFS)):
        d_out = torch.full((total + 32,), FILL, dtype=torch.uint8, device="cuda")
        out, out_off, rerr, dec, st = gather(torch, frame, info, offsets, lengths, cap, 2, max_blocks=m, d_out=d_out[:room])
        assert (st, dec, out_off) == (want, count, want_off) and rerr == [want] * len(offsets)
        assert (d_out.cpu().numpy() == FILL).all()


def test_a_damaged_block_and_a_wrong_dictionary(torch, frames):
    frame, info, host = frames("b70", 3)
    data = G.content("b70")
    offsets, lengths, cap = G.range_lists("b70")["word_edges"]
    for victim in (32, 33):                               # a stored block, a stream
        bad = frame.clone()
        entry = G.W3.blocks(host)[victim]
        bad[entry["payload_off"] + 9] ^= 0x40
        got = gather(torch, bad, info, offsets, lengths, cap, 3)
        errs = {e for e, (a, c) in zip(got[2], zip(offsets, lengths)) if victim in G.covering(a, c)}
        assert len(errs) == 1 and 0 not in errs and (victim != 32 or errs == {E.EILSEQ})
        check(got, data, offsets, lengths, cap, victim, {victim}, errs.pop())
    out, out_off, rerr, dec, st = gather(torch, frame, info, offsets, lengths, cap, 3, dictionary=G.dct()[:-1])
    want_off = G.model(data, offsets, lengths, cap)[1]
    assert (st, dec, out_off) == (E.EILSEQ, 0, want_off) and rerr == [E.EILSEQ] * len(offsets) and (out == FILL).all()


def test_the_old_calls_refuse_what_they_refused(torch, frames):
    from sqz_amd import frame as F
    frame, info, _ = frames("mixed", 3)
    part, err, st = F.read_frame(frame, 100, 50, info=info)              # sqz_hip_frame_read on a version-3 frame
    torch.cuda.synchronize()
    assert int(st.item()) == E.EINVAL
    out, out_off, rerr, dec, st = gather(torch, frame, info, [100], [50], 50, 2)     # and the gather without a dictionary
    assert (st, dec, rerr) == (E.EINVAL, 0, [E.EINVAL]) and (out == FILL).all()
    with pytest.raises(ValueError):
        F.gather_frame(frame, [len(G.content("mixed"))], [1], info=info, dictionary=G.dct())
    with pytest.raises(ValueError):
        F.gather_frame(frame, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                       info=info, dictionary=G.dct())
