"""CPU: the ABI surface of SQZF version 3 in the device-resident flavour and of the ranged read from a resident frame
(include/sqz/sqz.h): the scratch calls against the formulas the header states, every refusal that is decided before
the device is touched, and ENODEV behind them on a machine without one.  The pointers are never followed here."""
import errno

import pytest

STORED, DICT = 1, 2
E = errno.EINVAL
P = 0x7F0000001000          # a well-aligned address no call here gets as far as using


@pytest.fixture(scope="module")
def lib():
    from sqz_amd import build, _native
    build.build_native()
    return _native.lib()


def up256(n):
    return (n + 255) // 256 * 256


def test_scratch_calls_follow_their_formulas(lib):
    for content, bits in ((0, 12), (1, 12), (8904, 12), (8904, 13), (1 << 20, 12), ((1 << 26) + 5, 18), (5000, 24)):
        for D in (1, 3, 3000, 32767):
            index = 256 + 2 * up256(4 * (D + 64))
            for flags in (0, STORED, DICT, DICT | STORED):
                want = lib.sqz_hip_frame_scratch_bytes_ex(content, bits, 1, flags & STORED) + index
                assert lib.sqz_hip_frame_scratch_bytes_dict(content, bits, 1, flags, D) == want, (content, bits, D, flags)
                assert lib.sqz_hip_frame_scratch_bytes_dict(content, bits, 0, flags, D) == \
                    lib.sqz_hip_frame_scratch_bytes(content, bits, 0)
    # a bad block_bits, a flag that is none, a dictionary that cannot be
    for bits in (11, 25):
        assert lib.sqz_hip_frame_scratch_bytes_dict(100, bits, 1, DICT, 5) == 0
        assert lib.sqz_hip_frame_scratch_bytes_dict(100, bits, 0, DICT, 5) == 0
        assert lib.sqz_hip_frame_read_scratch_bytes(100, bits) == 0
    for flags in (4, DICT | 4, 0x80, 0x100 | DICT):
        assert lib.sqz_hip_frame_scratch_bytes_dict(100, 12, 1, flags, 5) == 0
        assert lib.sqz_hip_frame_scratch_bytes_dict(100, 12, 0, flags, 5) == 0
    for D in (0, 32768):
        assert lib.sqz_hip_frame_scratch_bytes_dict(100, 12, 1, DICT, D) == 0
    # the calls there were answer as they did
    for flags in (DICT, DICT | STORED):
        assert lib.sqz_hip_frame_scratch_bytes_ex(100, 12, 1, flags) == 0


def test_read_scratch_is_the_worst_case_over_every_offset(lib):
    for bits in (12, 13, 18):
        bb = 1 << bits
        for length in (0, 1, 2, bb - 1, bb, bb + 1, bb + 2, 16 * bb, 16 * bb + 2, 65536):
            k = 0 if length == 0 else ((length + bb - 2) >> bits) + 1
            # the most blocks any offset makes a range of this length cover
            if length > 0:
                assert k == max((((at + length - 1) >> bits) - (at >> bits) + 1) for at in (0, 1, bb - 1, bb - 2, bb // 2))
            want = lib.sqz_hip_frame_scratch_bytes(k << bits, bits, 0) + up256((k << bits) + 16) + 256
            assert lib.sqz_hip_frame_read_scratch_bytes(length, bits) == want, (bits, length)


def encode_dict(lib, d_in=P, content=8904, wb=15, bb=12, flags=DICT, parse=0, dct=P, D=3000, frame=P, cap=1 << 20,
                fbytes=P, status=P, err=P, scratch=P, sbytes=1 << 30):
    return lib.sqz_hip_frame_encode_dict(d_in, content, wb, bb, flags, parse, dct, D, frame, cap, fbytes, status, err,
                                         scratch, sbytes, None)


def decode_dict(lib, frame=P, avail=1 << 20, n=3, content=8904, dct=P, D=3000, out=P, err=P, status=P, scratch=P,
                sbytes=1 << 30):
    return lib.sqz_hip_frame_decode_dict(frame, avail, n, content, dct, D, out, err, status, scratch, sbytes, None)


def read(lib, frame=P, avail=1 << 20, n=3, content=8904, bits=12, at=4090, length=12, out=P, err=P, status=P, scratch=P,
         sbytes=1 << 30):
    return lib.sqz_hip_frame_read(frame, avail, n, content, bits, at, length, out, err, status, scratch, sbytes, None)


def read_dict(lib, frame=P, avail=1 << 20, n=3, content=8904, bits=12, at=4090, length=12, dct=P, D=3000, out=P, err=P,
              status=P, scratch=P, sbytes=1 << 30):
    return lib.sqz_hip_frame_read_dict(frame, avail, n, content, bits, at, length, dct, D, out, err, status, scratch,
                                       sbytes, None)


def test_call_level_refusals_need_no_device(lib):
    # the dictionary
    for call in (encode_dict, decode_dict, read_dict):
        assert call(lib, dct=None) == E and call(lib, D=0) == E and call(lib, D=32768) == E
        assert call(lib, frame=P + 8) == E and call(lib, scratch=P + 4) == E and call(lib, frame=None) == E
        assert call(lib, scratch=None) == E and call(lib, status=None) == E
    assert encode_dict(lib, wb=10, D=1024) == E             # window - 1 is the most
    assert encode_dict(lib, wb=12, D=4096) == E
    # the encode's own arguments
    assert encode_dict(lib, parse=2) == E and encode_dict(lib, flags=4) == E and encode_dict(lib, flags=DICT | 8) == E
    assert encode_dict(lib, wb=9) == E and encode_dict(lib, wb=16) == E and encode_dict(lib, bb=11) == E
    assert encode_dict(lib, bb=25) == E and encode_dict(lib, d_in=None) == E and encode_dict(lib, fbytes=None) == E
    assert encode_dict(lib, err=None) == E
    # the decode's
    assert decode_dict(lib, out=None) == E and decode_dict(lib, err=None) == E
    assert decode_dict(lib, n=0) == E and decode_dict(lib, n=3, content=0) == E and decode_dict(lib, n=4, content=8192) == E
    assert decode_dict(lib, avail=32 + 24 + 7) == errno.E2BIG       # header, index AND record
    # the reads'
    for call in (read, read_dict):
        assert call(lib, frame=P + 8) == E and call(lib, scratch=P + 4) == E and call(lib, status=None) == E
        assert call(lib, at=8904, length=1) == E and call(lib, at=8905, length=0) == E      # the range leaves the content
        assert call(lib, at=8000, length=905) == E and call(lib, at=0, length=8905) == E
        assert call(lib, at=1 << 63, length=1 << 63) == E
        assert call(lib, bits=11) == E and call(lib, bits=25) == E
        assert call(lib, n=2) == E and call(lib, n=4) == E and call(lib, bits=13) == E      # n is not ceil(content / block)
        assert call(lib, out=None) == E and call(lib, err=None) == E
    # the calls there were keep refusing the flag
    for flags in (DICT, DICT | STORED):
        assert lib.sqz_hip_frame_encode_ex(P, 100, 15, 18, flags, P, 1 << 20, P, P, P, P, 1 << 30, None) == E
        assert lib.sqz_hip_frame_encode_parse(P, 100, 15, 18, flags, 0, P, 1 << 20, P, P, P, P, 1 << 30, None) == E


def test_good_arguments_reach_the_device_and_find_none(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for flags in (0, STORED, DICT, DICT | STORED):
        for parse in (0, 1):
            assert encode_dict(lib, flags=flags, parse=parse) == errno.ENODEV
    assert encode_dict(lib, wb=10, D=1023) == errno.ENODEV and encode_dict(lib, content=0, d_in=None, err=None) == errno.ENODEV
    assert decode_dict(lib) == errno.ENODEV and decode_dict(lib, D=32767) == errno.ENODEV
    assert decode_dict(lib, n=0, content=0, out=None, err=None, avail=48) == errno.ENODEV
    for call in (read, read_dict):
        assert call(lib) == errno.ENODEV
        assert call(lib, at=0, length=8904) == errno.ENODEV and call(lib, at=8903, length=1) == errno.ENODEV
        assert call(lib, at=8904, length=0, out=None, err=None) == errno.ENODEV      # (the status is set on the stream)


def test_python_side_checks_the_dictionary_before_anything_native(lib, monkeypatch):
    import torch
    from sqz_amd import _native as N
    from sqz_amd import frame as F

    class Loud:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")

    info = {"n_blocks": 3, "content_bytes": 8904, "block_bytes": 4096, "win_bits": 10, "version": 3}
    frame = torch.zeros(64, dtype=torch.uint8)
    monkeypatch.setattr(N, "lib", lambda: Loud())
    for bad in (b"", bytes(1024), torch.zeros(1024, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8),
                torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            F.FrameEncoder(8904, 10, 12, dictionary=bad, device="cpu")
        with pytest.raises(ValueError):
            F.decode_frame(frame, torch.zeros(8904, dtype=torch.uint8), info=info, dictionary=bad)
        with pytest.raises(ValueError):
            F.read_frame(frame, 0, 10, info=info, dictionary=bad)
