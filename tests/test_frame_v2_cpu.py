"""CPU: SQZF version 2 (stored blocks) as the host side of the library reads it -- sqz_frame_info, sqz_frame_blocks,
sqz_frame_bound_ex: no device is touched -- held against the independent version-2 writer (tests/frame_writer_v2.py:
struct + zlib.crc32 + the CPU oracle per block, the outcome of every case fixed beforehand)."""
import ctypes as C
import errno

import pytest

import frame_writer as W
import frame_writer_v2 as W2


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


@pytest.mark.parametrize("name", W2.CASE_IDS)
def test_info_and_blocks_return_the_writers_fields(lib, name):
    for frame, version, flags in ((W2.case_frame(name), 2, W2.STORED), (W2.case_frame_v1(name), 1, 0)):
        want = W2.fields(frame)
        assert want["version"] == version and want["frame_bytes"] == len(frame)
        for avail in (32, len(frame)):
            rc, got, reserved = info(lib, frame, avail)
            assert rc == 0 and got == want and reserved == flags, (name, version, avail)
        rc, got = blocks(lib, frame + b"next record")
        assert rc == 0 and got == W2.blocks(frame), (name, version)
        n = want["n_blocks"]
        if n >= 3:
            rc, got = blocks(lib, frame, 1, n - 2)
            assert rc == 0 and got == W2.blocks(frame)[1:n - 1]
            assert blocks(lib, frame, 1, n)[0] == errno.EINVAL           # a range that leaves the frame
            assert blocks(lib, frame, avail=32 + 8 * n - 1)[0] == errno.E2BIG
    # the version-2 frame holds the content of the blocks it says are stored, and is never the larger one
    frame, data = W2.case_frame(name), W2.case_data(name)
    bb = W2.fields(frame)["block_bytes"]
    for b, blk in enumerate(W2.blocks(frame)):
        if blk["stored"]:
            at = blk["payload_off"]
            assert frame[at:at + blk["content_bytes"]] == data[b * bb:b * bb + blk["content_bytes"]]
    assert len(frame) <= len(W2.case_frame_v1(name))


@pytest.mark.parametrize("name", ["mandrill_bmp_w10_b18", "x64_w15_b12"])
def test_refusals(lib, name):
    frame = W2.case_frame(name)
    assert info(lib, frame)[0] == 0
    seen = set()
    for what, bad, head_errno, full_errno in W2.refusals(frame):
        assert info(lib, bad, 32)[0] == head_errno, what
        assert info(lib, bad)[0] == full_errno, what
        assert blocks(lib, bad)[0] == full_errno, what
        seen.add(what)
    assert {"v2_flags_0", "v2_flags_2", "v2_flags_3", "stored_one_word_more", "stored_one_word_less",
            "stored_bit_flipped_stale_crc", "payload_bytes_plus_8"} <= seen
    for what, bad, head_errno, full_errno in W.refusals(frame):             # the version-1 set on a version-2 frame
        if what in ("version_2", "flags_1"):                                # (those two flips make no change here)
            continue
        assert info(lib, bad, 32)[0] == head_errno, what
        assert info(lib, bad)[0] == full_errno, what


def test_bound_ex(lib):
    S = W2.STORED
    for name, _, _, bits, n_blocks, _, _, _, size in W2.CASES:
        n = len(W2.case_data(name))
        got = lib.sqz_frame_bound_ex(n, bits, S)
        assert size <= got <= W2.pad16(32 + 8 * n_blocks) + W2.pad8(n), name
        assert len(W2.case_frame_v1(name)) <= lib.sqz_frame_bound_ex(n, bits, 0), name
    for bits in (12, 16, 18, 24):
        prev = 0
        bb = 1 << bits
        for n in [0, 1, 2, 7, 8, bb - 1, bb, bb + 1, 2 * bb - 1, 2 * bb, 2 * bb + 1, 5 * bb + 3, 1 << 30, (1 << 30) + 1]:
            got = lib.sqz_frame_bound_ex(n, bits, S)
            assert got % 8 == 0 and prev <= got <= W2.pad16(32 + 8 * -(-n // bb)) + W2.pad8(n) and got >= 32 + n, (bits, n)
            prev = got
            assert lib.sqz_frame_bound_ex(n, bits, 0) == lib.sqz_frame_bound(n, bits)
            assert got <= lib.sqz_frame_bound(n, bits)
    assert lib.sqz_frame_bound_ex(0, 18, S) == 32
    for bits in (11, 25):
        assert lib.sqz_frame_bound_ex(100, bits, S) == 0 and lib.sqz_frame_bound_ex(100, bits, 0) == 0


def test_unknown_flags_are_refused_by_every_ex_call(lib):
    n = C.c_uint64(0)
    buf = (C.c_uint8 * 4096)()
    for flags in (2, 3, 0x80, 0x100):
        assert lib.sqz_frame_bound_ex(100, 18, flags) == 0
        assert lib.sqz_hip_frame_scratch_bytes_ex(100, 18, 1, flags) == 0
        assert lib.sqz_frame_compress_ex(b"abc", 3, 15, 18, flags, buf, 4096, C.byref(n)) == errno.EINVAL
        # (refused before any pointer is looked at and before a device is asked for)
        assert lib.sqz_hip_frame_encode_ex(None, 0, 15, 18, flags, None, 0, None, None, None, None, 0, None) == errno.EINVAL
    for encode in (0, 1):
        assert lib.sqz_hip_frame_scratch_bytes_ex(1 << 20, 18, encode, 0) == lib.sqz_hip_frame_scratch_bytes(1 << 20, 18, encode)
    # a decode of either version needs what it always did; an encode that may store needs a mask more
    assert lib.sqz_hip_frame_scratch_bytes_ex(1 << 20, 18, 0, W2.STORED) == lib.sqz_hip_frame_scratch_bytes(1 << 20, 18, 0)
    assert lib.sqz_hip_frame_scratch_bytes_ex(1 << 20, 18, 1, W2.STORED) > lib.sqz_hip_frame_scratch_bytes(1 << 20, 18, 1)


def test_empty_content_needs_no_device(lib):
    """an empty version-2 frame is 32 bytes of header: the host flavour writes it without a GPU"""
    n = C.c_uint64(0)
    buf = (C.c_uint8 * 64)()
    assert lib.sqz_frame_compress_ex(None, 0, 15, 18, W2.STORED, buf, 64, C.byref(n)) == 0
    assert bytes(buf[:n.value]) == W2.case_frame("empty")
    assert lib.sqz_frame_compress_ex(None, 0, 15, 18, 0, buf, 64, C.byref(n)) == 0
    assert bytes(buf[:n.value]) == W.case_frame("empty")


def test_python_side(lib):
    import sqz_amd
    from sqz_amd import frame as F
    for name in ("mandrill_bmp_w10_b18", "laozi_w15_b12", "one_byte", "empty"):
        v2, v1 = W2.case_frame(name), W2.case_frame_v1(name)
        assert sqz_amd.frame_info(v2) == W2.fields(v2) == F.frame_info(v2[:32])
        assert set(sqz_amd.frame_info(v2)) == set(sqz_amd.frame_info(v1))
        assert sqz_amd.frame_blocks(v2) == W2.blocks(v2) and sqz_amd.frame_blocks(v1) == W2.blocks(v1)
    with pytest.raises(sqz_amd.SqzError) as ei:
        sqz_amd.frame_blocks(W2.refusals(W2.case_frame("x64_w15_b12"))[4][1])
    assert ei.value.errno == errno.EINVAL
    assert F.frame_bound(0, store=True) == 32 and F.frame_bound(1 << 20, 18, store=True) == 32 + 32 + (1 << 20)
    assert F.frame_bound(1 << 20, 18) == F.frame_bound(1 << 20, 18, store=False) == lib.sqz_frame_bound(1 << 20, 18)
    for fn in ("frame_blocks", "frame_bound"):
        assert callable(getattr(sqz_amd, fn)) and fn in sqz_amd.__all__


def test_blocks_tool(lib, tmp_path, capsys):
    from sqz_amd import frame as F
    frame = W2.case_frame("mandrill_bmp_w10_b18")
    p = tmp_path / "f.sqzf"
    p.write_bytes(frame)
    assert F.main(["blocks", str(p)]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    got = []
    for k, line in enumerate(lines):
        head, rest = line.split(": ")
        assert int(head) == k
        got.append({key: int(v) for key, v in (item.split("=") for item in rest.split())})
    assert got == W2.blocks(frame)
    assert F.main(["info", str(p)]) == 0                                    # the same keys as for version 1
    said = {k: int(v) for k, v in (line.split(": ") for line in capsys.readouterr().out.strip().splitlines())}
    assert said == W2.fields(frame)
