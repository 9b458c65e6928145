"""CPU: SQZF version 3 (a shared dictionary) as the host side of the library reads it -- sqz_frame_info,
sqz_frame_blocks, sqz_frame_dict, sqz_frame_bound_dict: no device is touched -- held against the independent
version-3 writer (tests/frame_writer_v3.py), and the model the writer stands on (tests/dict_model.py) held against
the oracle."""
import ctypes as C
import errno
import struct

import pytest

import dict_model as DM
import frame_writer as W
import frame_writer_v2 as W2
import frame_writer_v3 as W3
import oracle_lib as O


@pytest.fixture(scope="module")
def lib():
    from sqz_amd import build, _native
    build.build_native()
    return _native.lib()


@pytest.fixture(scope="module")
def lao():
    return O.corpus("laozi.txt")


@pytest.fixture(scope="module")
def frames(lao):
    """(dictionary, content, frame without stored blocks, frame with): 4 KB blocks, the last one ragged; the noise
    block in the middle is stored when the flag allows it"""
    dct = lao[:3000]
    data = lao[3000:7096] + W2.random_bytes(4096, 11) + lao[7096:8000]
    plain = W3.write_frame(data, 15, 12, dct)
    stored = W3.write_frame(data, 15, 12, dct, store=True)
    assert [b["stored"] for b in W3.blocks(stored)] == [0, 1, 0] and len(stored) < len(plain)
    return dct, data, plain, stored


def info(lib, frame: bytes, avail: int = None):
    from sqz_amd import _native as N
    fi = N.FrameInfo()
    rc = lib.sqz_frame_info(frame, len(frame) if avail is None else avail, C.byref(fi))
    return rc, {k: int(getattr(fi, k)) for k, _ in N.FrameInfo._fields_ if k != "reserved"}, int(fi.reserved)


def blocks(lib, frame: bytes, avail: int = None):
    from sqz_amd import _native as N
    n = struct.unpack_from("<I", frame, 24)[0]
    out = (N.FrameBlock * max(n, 1))()
    rc = lib.sqz_frame_blocks(frame, len(frame) if avail is None else avail, 0, n, out)
    return rc, [{k: int(getattr(out[b], k)) for k, _ in N.FrameBlock._fields_} for b in range(n)]


def record(lib, frame: bytes, avail: int = None):
    nb, crc = C.c_uint32(0xCCCCCCCC), C.c_uint32(0xCCCCCCCC)
    rc = lib.sqz_frame_dict(frame, len(frame) if avail is None else avail, C.byref(nb), C.byref(crc))
    return rc, nb.value, crc.value


def test_the_model_without_a_dictionary_is_the_oracle(lao):
    for window in (1 << 10, 1 << 15):
        for block in (lao[:3000], lao[4000:4100], b"", b"a", b"ab", b"abc", b"abcabcabcabc"):
            wb = window.bit_length() - 1
            assert DM.stream(b"", block, window) == O.encode(block, wb, header=False), (window, len(block))
            toks = DM.tokens(b"", block, window)
            assert (toks == O.tokens(block, window)).all() and DM.expand(toks) == block


def test_the_model_with_a_dictionary_round_trips_and_gains(lao):
    dct, block = lao[:4000], lao[4000:8000]
    for lazy in (False, True):
        toks = DM.tokens(dct, block, 1 << 15, lazy)
        assert DM.expand(toks, dct) == block
        assert any(s < 0 for _, _, _, s in DM.sources(toks, len(dct)))      # it does reach into the dictionary
        assert len(DM.stream(dct, block, 1 << 15, lazy)) < len(DM.stream(b"", block, 1 << 15, lazy))
    # the dictionary is the text in front: the block's stream is the tail of what the oracle writes for both --
    # in tokens (the entropy stage starts fresh, so only the token words can be compared)
    both = O.tokens(dct + block, 1 << 15)
    own = DM.tokens(dct, block, 1 << 15)
    assert len(own) > 10 and (both[-10:] == own[-10:]).all()


def test_info_blocks_and_record_are_the_writers(lib, frames):
    dct, data, plain, stored = frames
    for frame, flags in ((plain, W3.DICT), (stored, W3.DICT | W3.STORED)):
        want = W3.fields(frame)
        assert want["version"] == 3 and want["frame_bytes"] == len(frame) and want["payload_off"] == W3.pad16(32 + 24 + 8)
        head = {k: v for k, v in want.items() if k not in ("dict_bytes", "dict_crc")}
        for avail in (32, len(frame), len(frame) + 5):
            rc, got, reserved = info(lib, frame + b"12345", avail)
            assert rc == 0 and got == head and reserved == flags, avail
        rc, got = blocks(lib, frame + b"next record")
        assert rc == 0 and got == W3.blocks(frame)
        assert record(lib, frame) == (0, len(dct), want["dict_crc"])
        assert want["dict_bytes"] == len(dct)
    # versions 1 and 2 have no record
    v1 = W.write_frame(data, 15, 12)
    assert record(lib, v1)[0] == errno.EINVAL and record(lib, W2.write_frame(data, 15, 12))[0] == errno.EINVAL


def test_refusals(lib, frames):
    dct, data, plain, stored = frames
    E, n = errno.EINVAL, 3

    def flip(frame, at, fmt, value, reseal=False):
        b = bytearray(frame)
        struct.pack_into(fmt, b, at, value)
        return W3.reseal(b) if reseal else bytes(b)

    # version and flags: version 3 iff bit 1, no unknown bits; refused from the header alone
    for what, bad in (("v3_without_bit_1", flip(plain, 7, "<B", 0)), ("v3_stored_only", flip(plain, 7, "<B", 1)),
                      ("v3_bit_2", flip(plain, 7, "<B", 6)), ("v3_bit_7", flip(plain, 7, "<B", 0x82)),
                      ("v1_with_bit_1", flip(plain, 4, "<B", 1)), ("v2_with_bit_1", flip(plain, 4, "<B", 2)),
                      ("v2_with_bits_0_1", flip(stored, 4, "<B", 2)), ("v4", flip(plain, 4, "<B", 4))):
        for resealed in (bad, W3.reseal(bytearray(bad))):
            assert info(lib, resealed, 32)[0] == E, what
            assert info(lib, resealed)[0] == E and blocks(lib, resealed)[0] == E and record(lib, resealed)[0] == E, what
    v1 = W.write_frame(data, 15, 12)
    assert info(lib, flip(v1, 7, "<B", 2))[0] == E and info(lib, flip(v1, 4, "<B", 3))[0] == E
    # the record is under index_crc: a flipped dict_bytes, a flipped dict_crc
    for at in (32 + 8 * n, 32 + 8 * n + 5):
        bad = bytearray(plain)
        bad[at] ^= 0x04
        assert info(lib, bytes(bad), 32)[0] == 0                            # (the header alone is consistent)
        assert info(lib, bytes(bad))[0] == errno.EILSEQ and blocks(lib, bytes(bad))[0] == errno.EILSEQ
        assert record(lib, bytes(bad))[0] == errno.EILSEQ
    # under a checksum that is right: a dictionary no window admits
    for nb in (0, 1 << 15, 0xFFFFFFFF):
        assert info(lib, flip(plain, 32 + 8 * n, "<I", nb, reseal=True))[0] == E, nb
    assert info(lib, flip(plain, 32 + 8 * n, "<I", (1 << 15) - 1, reseal=True))[0] == 0
    # a stored entry in a frame whose flags do not allow one
    assert info(lib, W3.reseal(bytearray(flip(stored, 7, "<B", W3.DICT))))[0] == E
    # a truncated record: the header is fine, the index is "not in reach" and nothing that needs it answers
    for avail in (32 + 8 * n, 32 + 8 * n + 7):
        assert info(lib, plain, avail)[0] == 0
        assert blocks(lib, plain, avail)[0] == errno.E2BIG and record(lib, plain, avail)[0] == errno.E2BIG
    assert record(lib, plain, W3.fields(plain)["payload_off"])[0] == 0
    assert info(lib, plain, 31)[0] == errno.E2BIG
    # the version-1 refusals on a version-3 frame
    for what, bad, head_errno, full_errno in W.refusals(plain):
        if what in ("version_2", "flags_1", "index_bit_flipped", "stream_words_sum", "content_bytes_changed"):
            continue                                                        # (covered above with the record in mind)
        assert info(lib, bad, 32)[0] == head_errno and info(lib, bad)[0] == full_errno, what


def test_bound_dict(lib, frames):
    dct, data, plain, stored = frames
    D, S = W3.DICT, W3.STORED
    assert len(plain) <= lib.sqz_frame_bound_dict(len(data), 12, D) == lib.sqz_frame_bound_dict(len(data), 12, 0)
    assert len(stored) <= lib.sqz_frame_bound_dict(len(data), 12, D | S) == W3.pad16(32 + 24 + 8) + W2.pad8(len(data))
    for bits in (12, 18):
        bb = 1 << bits
        for n in (0, 1, bb - 1, bb, bb + 1, 5 * bb + 3):
            blocks_n = -(-n // bb)
            shift = W3.pad16(32 + 8 * blocks_n + 8) - W3.pad16(32 + 8 * blocks_n)
            assert shift in (0, 16)
            for flags in (0, S):
                assert lib.sqz_frame_bound_dict(n, bits, flags | D) == lib.sqz_frame_bound_ex(n, bits, flags) + shift
    assert lib.sqz_frame_bound_dict(0, 18, D) == 48                         # header and record, padded
    for flags in (4, 0x80, 0x100):
        assert lib.sqz_frame_bound_dict(100, 18, flags) == 0
    assert lib.sqz_frame_bound_dict(100, 11, D) == 0 and lib.sqz_frame_bound_dict(100, 25, D) == 0


def test_calls_refuse_an_impossible_dictionary_before_any_device(lib):
    n64 = C.c_uint64(0)
    buf = (C.c_uint8 * 4096)()
    off = (C.c_uint64 * 2)(0, 3)
    err = (C.c_int32 * 1)()
    E = errno.EINVAL
    big = bytes(1 << 15)
    for dct, nb, window in ((None, 5, 1 << 15), (b"abc", 0, 1 << 15), (big, 1 << 15, 1 << 15), (big, 1 << 10, 1 << 10)):
        wb = window.bit_length() - 1
        assert lib.sqz_frame_compress_dict(b"abc", 3, wb, 12, 0, 0, dct, nb, buf, 4096, C.byref(n64)) == E
        assert lib.sqz_encode_blocks_dict(b"abc", off, 1, window, 0, dct, nb, buf, off, off, err) == E
        assert lib.sqz_hip_encode_blocks_dict(None, None, 0, window, 0, dct, nb, None, None, None, None, buf, 1 << 20, None) == E
        assert lib.sqz_hip_lz77_blocks_dict(None, None, 0, window, None, None, 1, 0, dct, nb, buf, 1 << 20, None) == E
    for dct, nb in ((None, 5), (b"abc", 0), (big, 1 << 15)):
        assert lib.sqz_decode_blocks_dict(b"abc", off, 1, dct, nb, buf, off, err) == E
        assert lib.sqz_hip_decode_blocks_dict(None, None, 0, dct, nb, None, None, None, None, 0, None) == E
    # the scan finder has no table, an unknown parse or flag is refused
    assert lib.sqz_hip_lz77_blocks_dict(None, None, 0, 1 << 15, None, None, 0, 0, b"abc", 3, buf, 1 << 20, None) == E
    assert lib.sqz_encode_blocks_dict(b"abc", off, 1, 1 << 15, 2, b"abc", 3, buf, off, off, err) == E
    assert lib.sqz_frame_compress_dict(b"abc", 3, 15, 12, 4, 0, b"abc", 3, buf, 4096, C.byref(n64)) == E
    # the device frame calls do not know the flag; sqz_frame_bound_ex answers as it always did
    for flags in (W3.DICT, W3.DICT | W3.STORED):
        assert lib.sqz_hip_frame_encode_ex(None, 0, 15, 18, flags, None, 0, None, None, None, None, 0, None) == E
        assert lib.sqz_hip_frame_encode_parse(None, 0, 15, 18, flags, 0, None, 0, None, None, None, None, 0, None) == E
        assert lib.sqz_hip_frame_scratch_bytes_ex(100, 18, 1, flags) == 0 and lib.sqz_frame_bound_ex(100, 18, flags) == 0
    # the index's share of the scratch, as the header says
    for nb in (1, 3, 1000, 32767):
        want = 256 + 2 * ((4 * (nb + 64) + 255) // 256 * 256)
        assert lib.sqz_hip_encode_scratch_bytes_dict(7, 12345, nb) == lib.sqz_hip_encode_scratch_bytes(7, 12345) + want
    assert lib.sqz_hip_encode_scratch_bytes_dict(0, 0, 32767) - lib.sqz_hip_encode_scratch_bytes(0, 0) == 262912


def test_empty_content_needs_no_device(lib):
    n = C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    for store in (False, True):
        assert lib.sqz_frame_compress_dict(None, 0, 15, 18, int(store), 0, b"abcde", 5, buf, 64, C.byref(n)) == 0
        assert bytes(buf[:n.value]) == W3.write_frame(b"", 15, 18, b"abcde", store=store) and n.value == 48
    assert lib.sqz_frame_compress_dict(None, 0, 15, 18, 0, 0, b"abcde", 5, buf, 40, C.byref(n)) == errno.E2BIG and n.value == 48
    out = (C.c_uint8 * 8)()
    frame = bytes(buf[:48])
    assert lib.sqz_frame_decompress_dict(frame, 48, b"abcde", 5, out, 8, C.byref(n), None) == 0 and n.value == 0
    assert lib.sqz_frame_decompress_dict(frame, 48, b"abcdf", 5, out, 8, C.byref(n), None) == errno.EILSEQ
    assert lib.sqz_frame_decompress_dict(frame, 48, b"abcd", 4, out, 8, C.byref(n), None) == errno.EILSEQ
    assert lib.sqz_frame_decompress(frame, 48, out, 8, C.byref(n), None) == errno.EINVAL
    assert lib.sqz_frame_read(frame, 48, 0, 0, out) == errno.EINVAL
    assert lib.sqz_frame_read_dict(frame, 48, b"abcde", 5, 0, 0, out) == 0


def test_python_side(lib, frames):
    import sqz_amd
    from sqz_amd import frame as F
    dct, data, plain, stored = frames
    got = sqz_amd.frame_info(plain)
    assert got == W3.fields(plain) and got["dict_bytes"] == len(dct)
    assert F.frame_info(plain[:32])["dict_bytes"] == 0                      # (the record is not in reach)
    v1 = W.write_frame(data, 15, 12)
    i1 = sqz_amd.frame_info(v1)
    assert i1 == W.fields(v1) and i1["dict_bytes"] == 0 and i1["dict_crc"] == 0
    assert F.frame_bound(1 << 20, 18, dictionary=True) == F.frame_bound(1 << 20, 18) + 16
    # a wrong length raises before anything native is called
    for bad in (b"", bytes(1 << 15)):
        with pytest.raises(ValueError):
            F.compress_frame(b"abc", dictionary=bad)
        with pytest.raises(ValueError):
            F.decompress_frame(plain, dictionary=bad)
        with pytest.raises(ValueError):
            F.read_range(plain, 0, 1, dictionary=bad)
    with pytest.raises(ValueError):
        F.compress_frame(b"abc", win_bits=10, dictionary=bytes(1024))
    from sqz_amd import batch
    for bad in (b"", bytes(1 << 15)):
        with pytest.raises(ValueError):
            batch.encode_blocks_host([b"abc"], 1 << 15, dictionary=bad)
        with pytest.raises(ValueError):
            batch.decode_blocks_host([b"12345678"], [3], dictionary=bad)


def test_info_tool_prints_the_record(lib, frames, tmp_path, capsys):
    from sqz_amd import frame as F
    dct, data, plain, stored = frames
    p = tmp_path / "a.sqzf"
    p.write_bytes(stored)
    assert F.main(["info", str(p)]) == 0
    out = capsys.readouterr().out
    assert f"dict_bytes: {len(dct)}" in out and f"dict_crc: {W3.fields(stored)['dict_crc']}" in out and "version: 3" in out
