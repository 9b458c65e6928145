"""GPU: append_frame -- more content behind a device-resident frame in one call -- on frames written by FrameEncoder:
the new frame against FrameEncoder's frame of old + data, against the independent writers' (tests/frame_append_cases.py),
and read back through decode_frame and gather_frame."""
import errno

import numpy as np
import pytest

import frame_append_cases as A
import frame_gather_cases as G

pytestmark = pytest.mark.gpu
E = errno
FILL = 0xA5
BB, BITS, WB = G.BB, G.BITS, G.WB
MOST = 310 * BB                              # the longest content any test encodes


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def dev(torch, data: bytes):
    return torch.from_numpy(np.frombuffer(bytes(data) + b"\0", np.uint8).copy())[:len(data)].cuda()


def dct_of(version):
    return G.dct() if version == 3 else None


@pytest.fixture(scope="module")
def encode(torch):
    """encode(version, parse, content) -> FrameEncoder's frame of it, one encoder per kind of frame, each frame once"""
    from sqz_amd import frame as F
    encoders, made = {}, {}

    def run(version, parse, content):
        key = (version, parse, content)
        if key not in made:
            if key[:2] not in encoders:
                encoders[key[:2]] = F.FrameEncoder(MOST, WB, BITS, store=version >= 2, parse=parse,
                                                   dictionary=dct_of(version))
            encoders[key[:2]].encode(dev(torch, content))
            made[key] = encoders[key[:2]].result()
        return made[key]
    return run


@pytest.fixture(scope="module")
def frames(torch, encode):
    """(name, version, parse) -> (device frame, info, host bytes) of an old content"""
    from sqz_amd import frame as F
    made = {}

    def get(name, version, parse="greedy"):
        key = (name, version, parse)
        if key not in made:
            host = encode(version, parse, A.old_content(name))
            info = F.frame_info(host)
            assert info["version"] == version and info["content_bytes"] == len(A.old_content(name))
            made[key] = (dev(torch, host + bytes(16))[:len(host)], info, host)
        return made[key]
    return get


def append(torch, frame, info, data, version, dictionary="default", room=None, **kw):
    """(the whole of d_out, frame_bytes, blocks_encoded, status) after a synchronise"""
    from sqz_amd import frame as F
    if dictionary == "default":
        dictionary = dct_of(version)
    if room is None:
        room = int(F.frame_bound(info["content_bytes"] + len(data), BITS, store=version >= 2, dictionary=version == 3)) + 32
    d_out = torch.full((max(room, 16),), FILL, dtype=torch.uint8, device="cuda")[:room]
    out, fb, enc, st = F.append_frame(frame, data, d_out=d_out, info=info, dictionary=dictionary, **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), int(fb.item()), int(enc.item()), int(st.item())


def untouched(got):
    return bool((got[0] == FILL).all())


def new_frame(got, what=None):
    out, fb, _, st = got
    assert st == 0 and fb > 0, (what, st)
    assert (out[fb:] == FILL).all(), what                # nothing behind frame_bytes is written
    return out[:fb].tobytes()


def read_back(torch, new, content, version, what):
    """decode_frame and gather_frame take the new frame as it is"""
    from sqz_amd import frame as F
    d_new = dev(torch, new + bytes(16))[:len(new)]
    back = torch.full((len(content) + 16,), FILL, dtype=torch.uint8, device="cuda")
    err, st = F.decode_frame(d_new, back, dictionary=dct_of(version))
    size = len(content)
    offsets = [o for o in (0, max(size - 5000, 0), max(size - 7, 0)) if size]
    lengths = [min(n, size - o) for o, n in zip(offsets, (9, 4999, 7))]
    out, out_off, rerr, dec, gst = F.gather_frame(d_new, offsets, lengths, dictionary=dct_of(version))
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and not err.cpu().numpy().any(), what
    assert back.cpu().numpy()[:size].tobytes() == content and (back.cpu().numpy()[size:] == FILL).all(), what
    assert int(gst.item()) == 0 and not rerr.cpu().numpy().any(), what
    assert out.cpu().numpy()[:sum(lengths)].tobytes() == b"".join(content[o:o + n] for o, n in zip(offsets, lengths)), what


KINDS = [(1, "greedy"), (2, "greedy"), (3, "greedy"), (1, "lazy"), (2, "lazy"), (3, "lazy")]


@pytest.mark.parametrize("version,parse", KINDS, ids=[f"v{v}-{p}" for v, p in KINDS])
def test_every_case_against_the_encoder_the_writers_and_the_readers(torch, frames, encode, version, parse):
    for name, length in A.cases():
        frame, info, host = frames(name, version, parse)
        data = A.data_of(name, length)
        content = A.old_content(name) + data
        what = (version, parse, name, length)
        got = append(torch, frame, info, data, version, parse=parse)
        if name == "empty" and length == 0:              # an empty frame stays one
            assert (got[1], got[2], got[3]) == (len(host), 0, 0) and got[0][:len(host)].tobytes() == host, what
            continue
        new = new_frame(got, what)
        assert got[2] == A.shape(name, length)[3], what
        assert new == encode(version, parse, content), what
        # the independent writers' frame: the C oracle is the greedy parse, dict_model knows both
        if parse == "greedy" or version == 3:
            assert new == A.expected(name, length, version, parse == "lazy"), what
        if length == 0:
            assert new == host, what
        read_back(torch, new, content, version, what)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_two_appends_are_one_and_an_update_afterwards_is_the_encoders(torch, frames, encode, version):
    from sqz_amd import frame as F
    name = "short"
    frame, info, host = frames(name, version)
    old, data = A.old_content(name), A.data_of(name, A.fill(name) + 2 * BB + 77)
    one = new_frame(append(torch, frame, info, data, version))
    assert one == encode(version, "greedy", old + data)
    # cut inside the touched block, on its edge, one byte behind it, on a later edge and inside a later block
    for cut in (1, A.fill(name) - 1, A.fill(name), A.fill(name) + 1, A.fill(name) + BB, A.fill(name) + BB + 100):
        first = new_frame(append(torch, frame, info, data[:cut], version))
        d_first = dev(torch, first + bytes(16))[:len(first)]
        assert new_frame(append(torch, d_first, F.frame_info(first), data[cut:], version)) == one, (version, cut)
    # ranges across the seam and in the new blocks, written into the appended frame
    d_one, size = dev(torch, one + bytes(16))[:len(one)], len(old) + len(data)
    offsets, lengths = [len(old) - 20, size - 90, len(old) + BB], [50, 90, 10]
    parts = [bytes([0x31 + k]) * n for k, n in enumerate(lengths)]
    patched = bytearray(old + data)
    for o, p in zip(offsets, parts):
        patched[o:o + len(p)] = p
    out, fb, _, rerr, _, st = F.update_frame(d_one, offsets, lengths, b"".join(parts), dictionary=dct_of(version))
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and not rerr.cpu().numpy().any()
    assert out[:int(fb.item())].cpu().numpy().tobytes() == encode(version, "greedy", bytes(patched))


def test_a_data_tensor_no_data_and_the_empty_frame(torch, frames, encode):
    from sqz_amd import frame as F
    for version in (1, 2, 3):
        frame, info, host = frames("mixed", version)
        data = A.data_of("mixed", 5000)
        want = encode(version, "greedy", A.old_content("mixed") + data)
        assert new_frame(append(torch, frame, info, dev(torch, data), version)) == want
        assert new_frame(append(torch, frame, info, np.frombuffer(data, np.uint8), version)) == want
        # d_out and info made by the call
        out, fb, enc, st = F.append_frame(frame, data, dictionary=dct_of(version))
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and out[:int(fb.item())].cpu().numpy().tobytes() == want and int(enc.item()) == 2
        # no data: the old frame's exact bytes, nothing encoded
        for nothing in (b"", dev(torch, b"")):
            got = append(torch, frame, info, nothing, version)
            assert new_frame(got) == host and got[2] == 0
        # the empty frame: 32 bytes, 48 with a dictionary's record; the result is the encoder's frame of the data
        empty, e_info, e_host = frames("empty", version)
        assert len(e_host) == (48 if version == 3 else 32) and e_info["n_blocks"] == 0
        for n in (1, BB, BB + 1):
            assert new_frame(append(torch, empty, e_info, data[:n], version)) == encode(version, "greedy", data[:n]), (version, n)


def test_the_refusals_in_their_order_leave_the_output_untouched(torch, frames):
    from sqz_amd import frame as F
    name, length = "short", A.fill("short") + BB + 904
    data = A.data_of(name, length)
    m = A.shape(name, length)[3]
    # a wrong and a missing dictionary; a dictionary for a frame that has none
    frame, info, host = frames(name, 3)
    got = append(torch, frame, info, data, 3, dictionary=G.dct()[:-1], room=64)
    assert (got[3], got[2], got[1]) == (E.EILSEQ, 0, 0) and untouched(got)
    got = append(torch, frame, info, data, 3, dictionary=None, room=64)
    assert (got[3], got[2], got[1]) == (E.EINVAL, 0, 0) and untouched(got)
    frame2, info2, host2 = frames(name, 2)
    got = append(torch, frame2, info2, data, 2, dictionary=G.dct())
    assert (got[3], got[2], got[1]) == (E.EINVAL, 0, 0) and untouched(got)
    for version in (1, 2, 3):
        frame, info, host = frames(name, version)
        # a frame of another window than the caller says, in front of the touched block's damage and the capacity
        other = dict(info)
        other["win_bits"] = 14
        entries = G.block_entries(host, version)
        bad = frame.clone()
        bad[entries[-1]["payload_off"] + 9] ^= 0x40
        got = append(torch, bad, other, data, version, room=64)
        assert (got[3], got[2], got[1]) == (E.EINVAL, 0, 0) and untouched(got), version
        # a damaged touched block, in front of the capacity: the status a gather of one byte of that block reports
        got = append(torch, bad, info, data, version, room=64)
        rerr = F.gather_frame(bad, [3 * BB], [1], info=info, dictionary=dct_of(version))[2]
        torch.cuda.synchronize()
        assert got[3] == int(rerr[0].item()) != 0 and (got[2], got[1]) == (m, 0) and untouched(got), (version, got)
        # E2BIG one byte short, with the size it takes; then the exact size
        want = A.expected(name, length, version)
        got = append(torch, frame, info, data, version, room=len(want) - 1)
        assert (got[3], got[2], got[1]) == (E.E2BIG, m, len(want)) and untouched(got), version
        got = append(torch, frame, info, data, version, room=len(want))
        assert got[3] == 0 and got[0].tobytes() == want, version
    # a stored touched block that is damaged: the checksum is all there is
    for version in (2, 3):
        frame, info, host = frames("noise_tail", version)
        last = G.block_entries(host, version)[-1]
        assert last["stored"] == 1
        bad = frame.clone()
        bad[last["payload_off"] + 9] ^= 0x40
        got = append(torch, bad, info, data[:100], version)
        assert (got[3], got[2], got[1]) == (E.EILSEQ, 1, 0) and untouched(got), version


def test_a_damaged_kept_block_is_carried_over_and_blamed_by_a_decode(torch, frames):
    from sqz_amd import frame as F
    for version, name, victim in ((1, "short", 1), (2, "short", 1), (3, "b70", 40), (2, "whole", 3)):
        frame, info, host = frames(name, version)
        data = A.data_of(name, A.fill(name) + BB + 904)
        content = A.old_content(name) + data
        bad = frame.clone()
        bad[G.block_entries(host, version)[victim]["payload_off"] + 9] ^= 0x40
        new = new_frame(append(torch, bad, info, data, version))
        back = torch.zeros(len(content), dtype=torch.uint8, device="cuda")
        err, st = F.decode_frame(dev(torch, new + bytes(16))[:len(new)], back, dictionary=dct_of(version))
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and [b for b, e in enumerate(err.cpu().tolist()) if e != 0] == [victim], (version, name)
        got = back.cpu().numpy().tobytes()
        assert got[:victim * BB] == content[:victim * BB] and got[(victim + 1) * BB:] == content[(victim + 1) * BB:]


def test_the_file_tool_appends(torch, tmp_path, capsys):
    from sqz_amd import frame as F
    x, y = A.old_content("short"), A.data_of("short", A.fill("short") + BB + 904)
    paths = {k: str(tmp_path / k) for k in ("x", "y", "xy", "dict", "fx", "fxy", "want", "back")}
    for key, blob in (("x", x), ("y", y), ("xy", x + y), ("dict", G.dct())):
        with open(paths[key], "wb") as fh:
            fh.write(blob)
    for flags in ([], ["--store"], ["--store", "--dict", paths["dict"]], ["--lazy", "--dict", paths["dict"]]):
        kind = ["--win-bits", str(WB), "--block-bits", str(BITS)] + flags
        rest = [f for f in flags if f != "--store"]
        with_dict = rest[rest.index("--dict"):][:2] if "--dict" in rest else []
        assert F.main(["c", paths["x"], paths["fx"]] + kind) == 0
        assert F.main(["c", paths["xy"], paths["want"]] + kind) == 0
        assert F.main(["a", paths["fx"], paths["y"], paths["fxy"]] + rest) == 0
        with open(paths["fxy"], "rb") as got, open(paths["want"], "rb") as want:
            assert got.read() == want.read(), flags
        assert F.main(["d", paths["fxy"], paths["back"]] + with_dict) == 0
        with open(paths["back"], "rb") as fh:
            assert fh.read() == x + y, flags
    # a status is the tool's one-line error and 1: a version-3 frame without its dictionary
    capsys.readouterr()
    assert F.main(["a", paths["fx"], paths["y"], paths["fxy"]]) == 1
    assert capsys.readouterr().out.startswith("sqz_amd.frame: ")
