"""CPU: SQZF version 4 (the byte-shuffle filter) as the host side of the library reads it -- sqz_frame_info,
sqz_frame_blocks, sqz_frame_elem, sqz_frame_bound_shuf, the scratch formulas and every call-level refusal: no device
is touched -- held against the independent version-4 writer (tests/frame_writer_v4.py: a numpy transposition, the CPU
oracle per block, struct + zlib.crc32), and the payload table of README / DESIGN.md on the CPU model."""
import ctypes as C
import errno
import os

import pytest

import frame_writer as W
import frame_writer_v4 as W4
import oracle_lib as O

E = errno.EINVAL
GOLDEN = os.path.join(O.GOLD, "ramp_u32.w15.b12.e4.sqzf")


@pytest.fixture(scope="module")
def lib():
    from sqz_amd import build, _native
    build.build_native()
    return _native.lib()


def info(lib, frame: bytes, avail: int = None):
    from sqz_amd import _native as N
    fi = N.FrameInfo()
    rc = lib.sqz_frame_info(frame, len(frame) if avail is None else avail, C.byref(fi))
    return rc, {k: int(getattr(fi, k)) for k, _ in N.FrameInfo._fields_ if k != "reserved"}, int(fi.reserved)


def blocks(lib, frame: bytes, first: int = 0, count: int = None, avail: int = None):
    from sqz_amd import _native as N
    n = W.fields(frame)["n_blocks"]
    count = n - first if count is None else count
    out = (N.FrameBlock * max(count, 1))()
    rc = lib.sqz_frame_blocks(frame, len(frame) if avail is None else avail, first, count, out)
    return rc, [{k: int(getattr(out[b], k)) for k, _ in N.FrameBlock._fields_} for b in range(count)]


def elem(lib, frame: bytes, avail: int = None):
    eb = C.c_uint32(77)
    return lib.sqz_frame_elem(frame, len(frame) if avail is None else avail, C.byref(eb)), eb.value


def frames():
    """(what, content, frame): both flags, every element size, ragged and whole and tiny contents, noise"""
    for name, e in W4.FIGURES:
        data = W4.figure_input(name)
        for store in (False, True):
            yield (name, e, store), data, W4.write_frame(data, 15, 12, e, store)
    ramp = W4.figure_input("u32_ramp")
    for e in W4.ELEMS:
        for n in (0, 1, e - 1, e, 4096, 4097):
            yield ("ramp", e, n), ramp[:n], W4.write_frame(ramp[:n], 12, 12, e, True)
    yield ("b13",), ramp, W4.write_frame(ramp, 15, 13, 4, False, True)


def test_the_writer_is_the_golden_frame_and_shuffles_as_stated():
    with open(GOLDEN, "rb") as fh:
        golden = fh.read()
    data = W4.figure_input("u32_ramp")
    assert len(data) == W4.FIGURE_BYTES == 16389
    assert golden == W4.write_frame(data, 15, 12, 4)         # the reference's own streams (tests/gen_golden_frame_v4.py)
    f = W4.fields(golden)
    assert (f["version"], f["flags"], f["elem_bytes"], f["zero"], f["n_blocks"]) == (4, 4, 4, 0, 5)
    assert f["payload_off"] == W4.pad16(32 + 8 * 5 + 8) and len(golden) == f["frame_bytes"]
    assert W4.shuffle(bytes(range(11)), 4) == bytes([0, 4, 1, 5, 2, 6, 3, 7, 8, 9, 10])
    assert W4.shuffle(bytes(range(7)), 2) == bytes([0, 2, 4, 1, 3, 5, 6]) and W4.shuffle(b"abc", 8) == b"abc"
    for e in W4.ELEMS:
        assert W4.unshuffle(W4.shuffle(data[:4097], e), e) == data[:4097]
    assert len(W4.write_frame(b"", 15, 12, 4)) == 48         # empty content: header, record, padding


def test_info_blocks_and_elem_return_the_writers_fields(lib):
    for what, data, frame in frames():
        want = W4.fields(frame)
        flags, e = want.pop("flags"), want.pop("elem_bytes")
        assert want.pop("zero") == 0 and want["frame_bytes"] == len(frame) and want["version"] == 4, what
        for avail in (32, 32 + 8 * want["n_blocks"] + 7, len(frame)):
            rc, got, reserved = info(lib, frame, avail)
            assert rc == 0 and got == want and reserved == flags, (what, avail)
        rc, got = blocks(lib, frame + b"next record")
        assert rc == 0 and got == W4.blocks(frame), what
        assert elem(lib, frame) == (0, e), what
        assert elem(lib, frame, want["payload_off"] - 1) == (errno.E2BIG, 77)
        assert lib.sqz_frame_elem(frame, len(frame), None) == 0
        n = want["n_blocks"]
        if n >= 3:
            rc, got = blocks(lib, frame, 1, n - 2)
            assert rc == 0 and got == W4.blocks(frame)[1:n - 1]
            assert blocks(lib, frame, 1, n)[0] == E
        # a stored block carries the caller's bytes, not the shuffled ones
        bb = want["block_bytes"]
        for b, blk in enumerate(W4.blocks(frame)):
            if blk["stored"]:
                at = blk["payload_off"]
                assert frame[at:at + blk["content_bytes"]] == data[b * bb:b * bb + blk["content_bytes"]]
    # the ragged 5-byte block is smaller than an element of 8 bytes and is stored under `store`
    assert W4.blocks(W4.write_frame(W4.figure_input("u64_stamps"), 15, 12, 8, True))[4]["stored"] == 1
    for frame in (W.case_frame("laozi_w15_b12"),):           # versions 1..3 have no such record
        assert elem(lib, frame) == (E, 77)


def test_every_malformed_variant(lib):
    frame = W4.write_frame(W4.figure_input("i16_sine_noise"), 15, 12, 2)
    assert info(lib, frame)[0] == 0
    seen = set()
    for what, bad, head_errno, full_errno in W4.refusals(frame):
        assert info(lib, bad, 32)[0] == head_errno, what
        assert info(lib, bad)[0] == full_errno, what
        assert blocks(lib, bad)[0] == full_errno, what
        assert elem(lib, bad)[0] == full_errno, what
        seen.add(what)
    assert {"v4_flags_0", "v4_flags_6", "v3_flags_4", "elem_bytes_3", "elem_bytes_16", "second_word_1",
            "record_stale_crc", "stored_entry_without_bit_0"} <= seen
    for what, bad, head_errno, full_errno in W.refusals(frame):                             # the version-1 set on a version-4 frame
        if what in ("version_2", "flags_1", "stream_words_sum", "index_bit_flipped", "content_bytes_changed"):
            continue                                         # (resealed without the record there: covered above)
        assert info(lib, bad, 32)[0] == head_errno and info(lib, bad)[0] == full_errno, what


def test_bound(lib):
    S, F4 = W4.STORED, W4.SHUFFLE
    for what, data, frame in frames():
        f = W4.fields(frame)
        bits = f["block_bytes"].bit_length() - 1
        for flags in (f["flags"], f["flags"] & S):           # SQZ_FRAME_SHUFFLE is implied
            assert len(frame) <= lib.sqz_frame_bound_shuf(len(data), bits, flags), what
    for bits in (12, 18, 24):
        bb = 1 << bits
        for n in [0, 1, 7, 8, bb - 1, bb, bb + 1, 2 * bb, 5 * bb + 3, 1 << 30]:
            blocks_n = -(-n // bb)
            assert lib.sqz_frame_bound_shuf(n, bits, F4 | S) == W4.pad16(32 + 8 * blocks_n + 8) + ((n + 7) & ~7)
            assert lib.sqz_frame_bound_shuf(n, bits, F4) == lib.sqz_frame_bound_shuf(n, bits, 0) == \
                lib.sqz_frame_bound(n, bits) - W4.pad16(32 + 8 * blocks_n) + W4.pad16(32 + 8 * blocks_n + 8)
    assert lib.sqz_frame_bound_shuf(0, 12, F4) == 48
    # the noise input under `store`: every block stored, the frame fits the bound exactly
    noise = W4.figure_input("u32_noise")
    frame = W4.write_frame(noise, 15, 12, 4, True)
    assert all(b["stored"] for b in W4.blocks(frame)) and len(frame) == lib.sqz_frame_bound_shuf(len(noise), 12, F4 | S)
    for flags in (2, 6, 8, 0x80, 0x100):
        assert lib.sqz_frame_bound_shuf(100, 12, flags) == 0
    for bits in (11, 25):
        assert lib.sqz_frame_bound_shuf(100, bits, F4) == 0
    for flags in (4, 5, 6):                                  # what the older calls said about flag 4 stays
        assert lib.sqz_frame_bound_ex(100, 18, flags) == 0 and lib.sqz_frame_bound_dict(100, 18, flags) == 0
        assert lib.sqz_hip_frame_scratch_bytes_ex(100, 18, 1, flags) == 0
        assert lib.sqz_hip_frame_scratch_bytes_dict(100, 18, 1, flags, 100) == 0


def up256(n):
    return (n + 255) & ~255


def test_scratch_formulas(lib):
    S, F4 = W4.STORED, W4.SHUFFLE
    for bits in (12, 18):
        for c in (0, 1, 4096, 16389, (1 << 20) + 5):
            for flags in (0, S, F4, F4 | S):
                assert lib.sqz_hip_frame_scratch_bytes_shuf(c, bits, 1, flags) == \
                    lib.sqz_hip_frame_scratch_bytes_ex(c, bits, 1, flags & S) + up256(c + 16), (bits, c, flags)
                assert lib.sqz_hip_frame_scratch_bytes_shuf(c, bits, 0, flags) == \
                    lib.sqz_hip_frame_scratch_bytes(c, bits, 0) + up256(c + 16), (bits, c, flags)
        bb = 1 << bits
        for length in (0, 1, 2, bb, bb + 1, 3 * bb + 7):
            k = 0 if length == 0 else ((length + bb - 2) >> bits) + 1
            assert lib.sqz_hip_frame_read_scratch_bytes_shuf(length, bits) == \
                lib.sqz_hip_frame_read_scratch_bytes(length, bits) + up256((k << bits) + 16), (bits, length)
    for bits in (11, 25):
        assert lib.sqz_hip_frame_scratch_bytes_shuf(100, bits, 1, F4) == 0
        assert lib.sqz_hip_frame_read_scratch_bytes_shuf(100, bits) == 0
    for flags in (2, 6, 8, 0x100):
        assert lib.sqz_hip_frame_scratch_bytes_shuf(100, 12, 1, flags) == 0
        assert lib.sqz_hip_frame_scratch_bytes_shuf(100, 12, 0, flags) == 0


def test_call_level_refusals_need_no_device(lib):
    """every one of these answers before a device is asked for (this test runs without one)"""
    L, F4 = lib, W4.SHUFFLE
    n = C.c_uint64(0)
    buf = (C.c_uint8 * 4096)()
    for eb in (0, 1, 3, 16):
        assert L.sqz_frame_compress_shuf(b"abcd", 4, 15, 12, F4, 0, eb, buf, 4096, C.byref(n)) == E
        assert L.sqz_hip_frame_encode_shuf(None, 0, 15, 12, F4, 0, eb, None, 0, None, None, None, None, 0, None) == E
        assert L.sqz_hip_frame_decode_shuf(None, 0, 0, 0, eb, None, None, None, None, 0, None) == E
        assert L.sqz_hip_frame_read_shuf(None, 0, 0, 0, 12, eb, 0, 0, None, None, None, None, 0, None) == E
        assert L.sqz_hip_shuffle_blocks(None, None, 0, eb, 0, None, None) == E
    for flags in (2, 3, 6, 7, 8, 0x100):                     # bit 1 (a dictionary) or an unknown bit
        assert L.sqz_frame_compress_shuf(b"abcd", 4, 15, 12, flags, 0, 4, buf, 4096, C.byref(n)) == E
        assert L.sqz_hip_frame_encode_shuf(None, 0, 15, 12, flags, 0, 4, None, 0, None, None, None, None, 0, None) == E
    for parse in (2, 7):                                     # a parse that is none
        assert L.sqz_frame_compress_shuf(b"abcd", 4, 15, 12, F4, parse, 4, buf, 4096, C.byref(n)) == E
        assert L.sqz_hip_frame_encode_shuf(None, 0, 15, 12, F4, parse, 4, None, 0, None, None, None, None, 0, None) == E
    for wb, bits in ((9, 12), (16, 12), (15, 11), (15, 25)):
        assert L.sqz_frame_compress_shuf(b"abcd", 4, wb, bits, F4, 0, 4, buf, 4096, C.byref(n)) == E
    # pointers: host memory stands in for device memory, nothing dereferences it before these checks
    raw = (C.c_uint8 * (1 << 16))()
    base = (C.addressof(raw) + 15) & ~15
    need = L.sqz_hip_frame_scratch_bytes_shuf(100, 12, 1, F4)
    words = (C.c_uint64 * 4)()
    status, err = (C.c_int32 * 1)(), (C.c_int32 * 4)()
    assert 0 < need < (1 << 15)
    frame_p, scratch_p, in_p = C.c_void_p(base), C.c_void_p(base + 16384), C.c_void_p(base + 8192)

    def enc(d_in=in_p, d_frame=frame_p, fb=words, st=status, er=err, scratch=scratch_p, scratch_bytes=need):
        return L.sqz_hip_frame_encode_shuf(d_in, 100, 15, 12, F4, 0, 4, d_frame, 4096, fb, st, er, scratch, scratch_bytes, None)
    assert enc(d_in=None) == E and enc(d_frame=None) == E and enc(fb=None) == E and enc(st=None) == E
    assert enc(er=None) == E and enc(scratch=None) == E
    assert enc(d_frame=C.c_void_p(base + 8)) == E and enc(scratch=C.c_void_p(base + 16384 + 4)) == E
    assert enc(scratch_bytes=need - 1) == E                  # a scratch one byte smaller than the formula
    need_d = L.sqz_hip_frame_scratch_bytes_shuf(100, 12, 0, F4)

    def dec(d_frame=frame_p, d_out=in_p, er=err, st=status, scratch=scratch_p, scratch_bytes=need_d, n_blocks=1, content=100):
        return L.sqz_hip_frame_decode_shuf(d_frame, 4096, n_blocks, content, 4, d_out, er, st, scratch, scratch_bytes, None)
    assert dec(d_frame=None) == E and dec(d_out=None) == E and dec(er=None) == E and dec(st=None) == E
    assert dec(scratch=None) == E and dec(d_frame=C.c_void_p(base + 4)) == E and dec(scratch=C.c_void_p(base + 16384 + 8)) == E
    assert dec(scratch_bytes=need_d - 1) == E and dec(n_blocks=0) == E and dec(n_blocks=1, content=0) == E
    assert L.sqz_hip_frame_decode_shuf(frame_p, 47, 1, 100, 4, in_p, err, status, scratch_p, need_d, None) == errno.E2BIG
    need_r = L.sqz_hip_frame_read_scratch_bytes_shuf(10, 12)

    def rd(d_frame=frame_p, d_out=in_p, er=err, st=status, scratch=scratch_p, bits=12, n_blocks=1, offset=0, length=10):
        return L.sqz_hip_frame_read_shuf(d_frame, 4096, n_blocks, 100, bits, 4, offset, length, d_out, er, st, scratch,
                                         need_r, None)
    assert rd(d_frame=None) == E and rd(d_out=None) == E and rd(er=None) == E and rd(st=None) == E and rd(scratch=None) == E
    assert rd(d_frame=C.c_void_p(base + 2)) == E and rd(bits=11) == E and rd(n_blocks=2) == E
    assert rd(offset=95, length=10) == E and rd(offset=101, length=0) == E
    off = (C.c_uint64 * 2)(0, 8)
    assert L.sqz_hip_shuffle_blocks(None, off, 1, 4, 0, in_p, None) == E
    assert L.sqz_hip_shuffle_blocks(in_p, None, 1, 4, 0, frame_p, None) == E
    assert L.sqz_hip_shuffle_blocks(in_p, off, 1, 4, 0, None, None) == E
    assert L.sqz_hip_shuffle_blocks(in_p, off, 1, 4, 0, in_p, None) == E    # in place is not on offer
    assert L.sqz_hip_shuffle_blocks(None, None, 0, 4, 1, None, None) == 0   # no ranges: nothing to do


def test_empty_content_needs_no_device(lib):
    n = C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    for flags, store in ((W4.SHUFFLE, False), (0, False), (W4.SHUFFLE | W4.STORED, True)):
        for e in W4.ELEMS:
            assert lib.sqz_frame_compress_shuf(None, 0, 15, 12, flags, 0, e, buf, 64, C.byref(n)) == 0
            assert bytes(buf[:n.value]) == W4.write_frame(b"", 15, 12, e, store) and n.value == 48
    assert lib.sqz_frame_compress_shuf(None, 0, 15, 12, W4.SHUFFLE, 0, 4, buf, 47, C.byref(n)) == errno.E2BIG
    out = (C.c_uint8 * 8)()
    frame = W4.write_frame(b"", 15, 12, 4)
    assert lib.sqz_frame_decompress_shuf(frame, len(frame), out, 8, C.byref(n), None) == 0 and n.value == 0
    assert lib.sqz_frame_read_shuf(frame, len(frame), 0, 0, out) == 0
    # the readers there were refuse a version-4 frame; the dictionary readers as well
    assert lib.sqz_frame_decompress(frame, len(frame), out, 8, C.byref(n), None) == E
    assert lib.sqz_frame_read(frame, len(frame), 0, 0, out) == E
    assert lib.sqz_frame_decompress_dict(frame, len(frame), b"abc", 3, out, 8, C.byref(n), None) == E
    assert lib.sqz_frame_read_dict(frame, len(frame), b"abc", 3, 0, 0, out) == E
    v3 = bytearray(frame)                                    # and the _shuf readers a version-3 one
    v3[4], v3[7] = 3, 2
    assert lib.sqz_frame_decompress_shuf(bytes(v3), len(v3), out, 8, C.byref(n), None) != 0


def test_python_side(lib, tmp_path, capsys):
    import sqz_amd
    from sqz_amd import frame as F
    frame = W4.write_frame(W4.figure_input("u64_stamps"), 15, 12, 8, True)
    want = W4.fields(frame)
    flags, zero = want.pop("flags"), want.pop("zero")
    got = sqz_amd.frame_info(frame)
    assert got == want and got["elem_bytes"] == 8 and "elem_bytes" in got
    head = F.frame_info(frame[:32])                          # the record is not in reach: 0
    assert head["elem_bytes"] == 0 and head["version"] == 4
    v1 = W.case_frame("laozi_w15_b12")
    assert "elem_bytes" not in sqz_amd.frame_info(v1) and sqz_amd.frame_info(v1)["elem_bytes"] == 0
    assert sqz_amd.frame_blocks(frame) == W4.blocks(frame)
    assert F.frame_bound(16389, 12, store=True, shuffle=8) == len(W4.write_frame(W4.figure_input("u32_noise"), 15, 12, 4, True))
    for bad in (1, 3, 16, -2, True, "4", 4.5, None):
        with pytest.raises(ValueError):
            F.compress_frame(b"abcdefgh", shuffle=bad)
        with pytest.raises(ValueError):
            F.FrameEncoder(64, 15, 12, device="cpu", shuffle=bad)
    with pytest.raises(ValueError):
        F.compress_frame(b"abcdefgh", shuffle=4, dictionary=b"abc")
    with pytest.raises(ValueError):
        F.FrameEncoder(64, 15, 12, device="cpu", shuffle=2, dictionary=b"abc")
    # shuffle=0 is the frame there always was: the golden version-1 frame, empty content here (no device)
    assert F.compress_frame(b"", 15, 12, shuffle=0) == W.write_frame(b"", 15, 12) == F.compress_frame(b"", 15, 12)
    assert F.compress_frame(b"", 15, 12, shuffle=4) == W4.write_frame(b"", 15, 12, 4)
    assert F.decompress_frame(W4.write_frame(b"", 15, 12, 4)) == b""
    # gather, update, append and the file tool's `a` refuse version 4 before anything native runs
    info = sqz_amd.frame_info(frame)
    for call in (lambda: F.gather_frame(None, [0], [1], info=info), lambda: F.update_frame(None, [0], [1], b"x", info=info),
                 lambda: F.append_frame(None, b"x", info=info), lambda: F._append_file(frame, b"x", None, "greedy")):
        with pytest.raises(ValueError, match="version-4"):
            call()
    p, q = tmp_path / "f.sqzf", tmp_path / "more"
    p.write_bytes(frame)
    q.write_bytes(b"more")
    assert F.main(["a", str(p), str(q), str(tmp_path / "out")]) == 1 and "version-4" in capsys.readouterr().out
    assert F.main(["info", str(p)]) == 0
    said = {k: int(v) for k, v in (line.split(": ") for line in capsys.readouterr().out.strip().splitlines())}
    assert said == want
    assert F.main(["blocks", str(p)]) == 0 and len(capsys.readouterr().out.strip().splitlines()) == 5
    e = tmp_path / "empty"
    e.write_bytes(b"")
    assert F.main(["c", str(e), str(tmp_path / "e.sqzf"), "--block-bits", "12", "--shuffle", "2"]) == 0
    assert (tmp_path / "e.sqzf").read_bytes() == W4.write_frame(b"", 15, 12, 2)
    assert F.main(["c", str(e), str(tmp_path / "e2.sqzf"), "--shuffle", "3"]) == 1
    assert F.main(["c", str(e), str(tmp_path / "e3.sqzf"), "--shuffle", "4", "--dict", str(q)]) == 1
    assert "shuffle_blocks" in sqz_amd.__all__ and callable(sqz_amd.shuffle_blocks)


def test_the_filter_shrinks_the_payload_of_the_numeric_inputs():
    """the table of README / DESIGN.md, on the CPU model; the noise input is NOT asserted"""
    table = {("u32_ramp", 12): (6584, 5064), ("u32_ramp", 13): (6544, 4920),
             ("f32_sine", 12): (15840, 12144), ("f32_sine", 13): (15528, 11656),
             ("i16_sine_noise", 12): (11864, 7872), ("i16_sine_noise", 13): (11568, 7456),
             ("u64_stamps", 12): (6160, 4784), ("u64_stamps", 13): (5944, 4896),
             ("u32_noise", 12): (17336, 17312), ("u32_noise", 13): (17048, 17016)}
    for name, e in W4.FIGURES:
        for bits in (12, 13):
            plain, shuffled = W4.model_payload(name, 0, bits), W4.model_payload(name, e, bits)
            print(name, e, bits, plain, shuffled)
            assert (plain, shuffled) == table[(name, bits)]
            if name != "u32_noise":
                assert shuffled < plain, (name, bits)
