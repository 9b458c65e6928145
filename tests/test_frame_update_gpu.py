"""GPU: update_frame -- many byte ranges written into a device-resident frame in one call -- on frames written by
FrameEncoder: the new frame against FrameEncoder's frame of the patched content, against the independent writers'
(tests/frame_update_cases.py), and read back through decode_frame and gather_frame."""
import errno

import numpy as np
import pytest

import frame_gather_cases as G
import frame_update_cases as U

pytestmark = pytest.mark.gpu
E = errno
FILL = 0xA5
LISTS = ("one", "zero", "to_the_end", "two_edges", "last_block", "two_in_one_block", "descending", "unaligned", "whole")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev(torch, data: bytes):
    return torch.from_numpy(np.frombuffer(bytes(data) + b"\0", np.uint8).copy())[:len(data)].cuda()


@pytest.fixture(scope="module")
def encoders(torch):
    """encode(name, version, parse, content) -> the frame's bytes, one FrameEncoder per kind of frame"""
    from sqz_amd import frame as F
    made = {}

    def encode(name, version, parse, content):
        key = (name, version, parse)
        if key not in made:
            made[key] = F.FrameEncoder(len(G.content(name)), G.WB, G.BITS, store=version >= 2, parse=parse,
                                       dictionary=G.dct() if version == 3 else None)
        made[key].encode(dev(torch, content))
        return made[key].result()
    return encode


@pytest.fixture(scope="module")
def frames(torch, encoders):
    """(name, version, parse) -> (device frame, info, host bytes), each encoded once"""
    from sqz_amd import frame as F
    made = {}

    def get(name, version, parse="greedy"):
        key = (name, version, parse)
        if key not in made:
            host = encoders(name, version, parse, G.content(name))
            info = F.frame_info(host)
            assert info["version"] == version and info["n_blocks"] == len(G.PATTERNS[name])
            made[key] = (dev(torch, host), info, host)
        return made[key]
    return get


def update(torch, frame, info, offsets, lengths, data, cap, version, dictionary="default", room=None, **kw):
    """(the whole of d_out, frame_bytes, data_off, range_err, blocks_encoded, status) after a synchronise"""
    from sqz_amd import frame as F
    if dictionary == "default":
        dictionary = G.dct() if version == 3 else None
    if room is None:
        room = int(F.frame_bound(info["content_bytes"], G.BITS, store=version >= 2, dictionary=version == 3)) + 32
    d_out = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
    out, fb, data_off, rerr, enc, st = F.update_frame(frame, offsets, lengths, data, max_length=cap, d_out=d_out, info=info,
                                                      dictionary=dictionary, **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), int(fb.item()), data_off.cpu().tolist(), rerr.cpu().tolist(), int(enc.item()), int(st.item())


def untouched(got):
    return bool((got[0] == FILL).all())


def new_frame(got, what=None):
    out, fb, _, _, _, st = got
    assert st == 0 and fb > 0, (what, st)
    assert (out[fb:] == FILL).all(), what
    return out[:fb].tobytes()


def _signed(torch, values):
    return torch.tensor([v - (1 << 64) if v >> 63 else v for v in values], dtype=torch.int64, device="cuda")


CASES = [(1, "mixed", "greedy", LISTS), (2, "mixed", "greedy", LISTS), (3, "mixed", "greedy", LISTS),
         (3, "mixed", "lazy", LISTS), (3, "short", "greedy", LISTS), (1, "b70", "greedy", ("word_edges", "many_65")),
         (2, "b300", "greedy", ("many_257", "word_edges")), (3, "b300", "greedy", ("many_257", "word_edges"))]


@pytest.mark.parametrize("version,name,parse,keys", CASES, ids=[f"v{v}-{n}-{p}" for v, n, p, _ in CASES])
def test_every_list_against_the_encoder_the_writers_and_the_readers(torch, frames, encoders, version, name, parse, keys):
    from sqz_amd import frame as F
    frame, info, host = frames(name, version, parse)
    content = G.content(name)
    dct = G.dct() if version == 3 else None
    for key in keys:
        offsets, lengths, cap = G.range_lists(name)[key]
        what = (version, name, parse, key)
        data, patched = U.data_of(name, offsets, lengths, cap), U.patched(name, offsets, lengths, cap)
        _, want_off, _, blocks = G.model(content, offsets, lengths, cap)
        got = update(torch, frame, info, offsets, lengths, data, cap, version, parse=parse)
        new = new_frame(got, what)
        assert got[2] == want_off and not any(got[3]) and got[4] == len(blocks), what
        assert new == encoders(name, version, parse, patched), what
        # the independent writer's frame: dict_model is slow Python, so version 3 only where a few blocks are patched;
        # the C oracle, which is the greedy parse, everywhere else
        if version < 3 or len(blocks) <= 12:
            assert new == U.frame_of(patched, version, parse == "lazy"), what
        d_new = dev(torch, new)
        back = torch.full((len(content) + 16,), FILL, dtype=torch.uint8, device="cuda")
        err, st = F.decode_frame(d_new, back, dictionary=dct)
        out, out_off, rerr, dec, gst = F.gather_frame(d_new, offsets, lengths, max_length=cap, dictionary=dct)
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and not err.cpu().numpy().any() and back.cpu().numpy()[:len(content)].tobytes() == patched, what
        assert int(gst.item()) == 0 and not rerr.cpu().numpy().any(), what
        assert out.cpu().numpy()[:len(data)].tobytes() == data and out_off.cpu().tolist() == want_off, what


def test_the_contents_own_bytes_no_range_and_a_data_tensor(torch, frames):
    for version, name in ((1, "mixed"), (2, "b300"), (3, "short")):
        frame, info, host = frames(name, version)
        content = G.content(name)
        offsets, lengths, cap = G.range_lists(name)["unaligned" if name != "b300" else "many_257"]
        own = b"".join(content[o:o + n] for o, n in zip(offsets, lengths))
        assert new_frame(update(torch, frame, info, offsets, lengths, own, cap, version)) == host
        assert new_frame(update(torch, frame, info, offsets, lengths, dev(torch, own), cap, version)) == host
        got = update(torch, frame, info, [], [], b"", 0, version)
        assert new_frame(got) == host and got[2] == [0] and got[4] == 0


def test_ranges_from_the_device_and_the_refusals_in_their_order(torch, frames):
    name, version = "b70", 2
    frame, info, host = frames(name, version)
    content = G.content(name)
    # offsets as device tensors, the invalid list: ERANGE, and which ranges
    o, ln, cap = G.range_lists(name)["invalid"]
    data = U.data_of(name, o, ln, cap)
    got = update(torch, frame, info, _signed(torch, o), _signed(torch, ln), data, cap, version)
    assert got[5] == E.ERANGE and got[1] == 0 and untouched(got)
    assert got[3] == [0, E.EINVAL, 0, E.EINVAL, 0, E.EINVAL, 0] and got[2] == G.model(content, o, ln, cap)[1]
    # the valid ones of them, from the device as well
    keep = [k for k in range(len(o)) if G.valid(o[k], ln[k], cap, len(content))]
    vo, vl = [o[k] for k in keep], [ln[k] for k in keep]
    got = update(torch, frame, info, _signed(torch, vo), _signed(torch, vl), data, cap, version)
    assert new_frame(got) == U.frame_of(U.patched(name, vo, vl, cap), version)
    # ENOBUFS with the distinct count, in front of ENODATA; ENODATA; E2BIG one byte short, then success
    o, ln, cap = G.range_lists(name)["word_edges"]
    data, patched = U.data_of(name, o, ln, cap), U.patched(name, o, ln, cap)
    count = len(G.model(content, o, ln, cap)[3])
    got = update(torch, frame, info, o, ln, data[:-1], cap, version, max_blocks=count - 1)
    assert (got[5], got[4], got[1]) == (E.ENOBUFS, count, 0) and untouched(got)
    got = update(torch, frame, info, o, ln, data[:-1], cap, version)
    assert (got[5], got[1]) == (E.ENODATA, 0) and untouched(got)
    want = U.frame_of(patched, version)
    got = update(torch, frame, info, o, ln, data, cap, version, room=len(want) - 1)
    assert (got[5], got[1]) == (E.E2BIG, len(want)) and untouched(got)
    got = update(torch, frame, info, o, ln, data, cap, version, room=len(want), max_blocks=count)
    assert got[5] == 0 and got[0].tobytes() == want


def test_a_wrong_dictionary_and_damaged_blocks(torch, frames):
    from sqz_amd import frame as F
    name, version = "b70", 3
    frame, info, host = frames(name, version)
    content = G.content(name)
    o, ln, cap = G.range_lists(name)["word_edges"]
    data = U.data_of(name, o, ln, cap)
    got = update(torch, frame, info, o, ln, data, cap, version, dictionary=G.dct()[:-1])
    assert (got[5], got[4], got[1]) == (E.EILSEQ, 0, 0) and untouched(got)
    got = update(torch, frame, info, o, ln, data, cap, 2)                       # and the call without one
    assert (got[5], got[4]) == (E.EINVAL, 0) and untouched(got)
    entries = G.W3.blocks(host)
    for victim in (32, 33):                                                  # a stored block, a stream: both touched
        bad = frame.clone()
        bad[entries[victim]["payload_off"] + 9] ^= 0x40
        got = update(torch, bad, info, o, ln, data, cap, version)
        # the status a gather of one byte of that block gives its range: the decoder's errno, else EILSEQ
        rerr = F.gather_frame(bad, [victim * G.BB], [1], info=info, dictionary=G.dct())[2]
        torch.cuda.synchronize()
        assert got[5] == int(rerr[0].item()) != 0 and (victim != 32 or got[5] == E.EILSEQ), (victim, got[5])
        assert got[1] == 0 and untouched(got)
    # a damaged KEPT block: status 0, and a decode of the new frame blames exactly that block
    victim = 40
    assert victim not in G.model(content, o, ln, cap)[3]
    bad = frame.clone()
    bad[entries[victim]["payload_off"] + 9] ^= 0x40
    new = new_frame(update(torch, bad, info, o, ln, data, cap, version))
    back = torch.zeros(len(content), dtype=torch.uint8, device="cuda")
    err, st = F.decode_frame(dev(torch, new), back, dictionary=G.dct())
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and [b for b, e in enumerate(err.cpu().tolist()) if e != 0] == [victim]
    patched = U.patched(name, o, ln, cap)
    got_back = back.cpu().numpy().tobytes()
    assert got_back[:victim * G.BB] == patched[:victim * G.BB] and got_back[(victim + 1) * G.BB:] == patched[(victim + 1) * G.BB:]


def test_overlapping_ranges_with_different_data(torch, frames):
    from sqz_amd import frame as F
    for version in (2, 3):
        frame, info, host = frames("short", version)
        content = G.content("short")
        offsets, lengths = [4000, 4050, 4090, 9000], [200, 100, 300, 50]         # three that overlap, across a block edge
        parts = [bytes([0x11 * (k + 1)]) * n for k, n in enumerate(lengths)]
        new = new_frame(update(torch, frame, info, offsets, lengths, b"".join(parts), 300, version))
        back = torch.zeros(len(content), dtype=torch.uint8, device="cuda")
        err, st = F.decode_frame(dev(torch, new), back, dictionary=G.dct() if version == 3 else None)
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and not err.cpu().numpy().any()                # every checksum holds
        got = back.cpu().numpy().tobytes()
        for at in range(len(content)):
            cands = {p[at - o] for o, n, p in zip(offsets, lengths, parts) if o <= at < o + n}
            assert got[at] in (cands or {content[at]}), at
