"""CPU: the SQZF frame format as the host side of the library reads it (sqz_frame_info, sqz_frame_bound: no
device is touched), held against an independent writer (tests/frame_writer.py: struct + zlib.crc32 + the CPU
oracle per block) and against a golden frame whose streams the compiled reference produced."""
import ctypes as C
import errno
import os

import pytest

import frame_writer as W
import oracle_lib as O

GOLDEN_FRAME = os.path.join(O.GOLD, "laozi.txt.w15.b12.sqzf")


@pytest.fixture(scope="module")
def lib():
    from sqz_amd import build, _native
    build.build_native()
    return _native.lib()


def info(lib, frame: bytes, avail: int = None):
    from sqz_amd import _native as N
    fi = N.FrameInfo()
    rc = lib.sqz_frame_info(frame, len(frame) if avail is None else avail, C.byref(fi))
    return rc, {k: int(getattr(fi, k)) for k, _ in N.FrameInfo._fields_ if k != "reserved"}


@pytest.mark.parametrize("name", W.CASE_IDS)
def test_info_returns_the_writers_fields(lib, name):
    _, _, wb, bits, size = next(c for c in W.CASES if c[0] == name)
    frame = W.case_frame(name)
    assert len(frame) == size                       # the writer's self-check: sizes measured independently
    want = W.fields(frame)
    assert want["win_bits"] == wb and want["block_bytes"] == 1 << bits and want["frame_bytes"] == size
    for avail in (32, len(frame)):
        rc, got = info(lib, frame, avail)
        assert rc == 0 and got == want, (name, avail)
    rc, got = info(lib, frame + b"next record")     # a frame may be followed by something else
    assert rc == 0 and got == want


def test_info_refusals(lib):
    frame = W.case_frame("laozi_w15_b12")
    assert info(lib, frame)[0] == 0
    seen = set()
    for name, bad, head_errno, full_errno in W.refusals(frame):
        assert info(lib, bad, 32)[0] == head_errno, name
        assert info(lib, bad)[0] == full_errno, name
        seen.add(name)
    assert {"magic", "version_2", "flags_1", "win_bits_9", "win_bits_16", "block_bits_11", "block_bits_25",
            "n_blocks_plus_one", "content_bytes_changed", "index_bit_flipped", "stream_words_sum"} <= seen
    assert info(lib, frame, 31)[0] == errno.E2BIG
    assert info(lib, frame, 0)[0] == errno.E2BIG
    from sqz_amd import _native as N
    assert lib.sqz_frame_info(None, 64, C.byref(N.FrameInfo())) == errno.EINVAL
    assert lib.sqz_frame_info(frame, len(frame), None) == errno.EINVAL


def test_bound(lib):
    for name, _, _, bits, size in W.CASES:
        n = len(W.case_data(name))
        assert lib.sqz_frame_bound(n, bits) >= size, name
    for bits in (12, 16, 18, 24):
        prev = 0
        bb = 1 << bits
        for n in [0, 1, 2, 7, 8, bb - 1, bb, bb + 1, 2 * bb - 1, 2 * bb, 2 * bb + 1, 5 * bb + 3, 1 << 30, (1 << 30) + 1]:
            got = lib.sqz_frame_bound(n, bits)
            assert got % 8 == 0 and got >= prev and got >= 32 + n, (bits, n)
            prev = got
    assert lib.sqz_frame_bound(0, 18) == 32
    assert lib.sqz_frame_bound(100, 11) == 0 and lib.sqz_frame_bound(100, 25) == 0


def test_golden_frame_from_the_compiled_reference(lib):
    """tests/golden/laozi.txt.w15.b12.sqzf: streams by the compiled reference (tests/gen_golden_frame.py).  It
    parses, and the independent writer over the CPU oracle reproduces it byte for byte."""
    with open(GOLDEN_FRAME, "rb") as fh:
        gold = fh.read()
    rc, got = info(lib, gold)
    assert rc == 0 and got == W.fields(gold)
    assert got["content_bytes"] == len(O.corpus("laozi.txt")) and got["win_bits"] == 15 and got["block_bytes"] == 4096
    assert W.case_frame("laozi_w15_b12") == gold


def test_python_side(lib):
    import sqz_amd
    from sqz_amd import frame as F
    frame = W.case_frame("confucius_w15_b14")
    assert sqz_amd.frame_info(frame) == W.fields(frame) == F.frame_info(frame[:32])
    with pytest.raises(sqz_amd.SqzError) as ei:
        sqz_amd.frame_info(b"SQZG" + frame[4:])
    assert ei.value.errno == errno.EINVAL
    assert F.frame_bound(0) == 32
    for fn in ("compress_frame", "decompress_frame", "frame_info", "read_range"):
        assert callable(getattr(sqz_amd, fn)) and fn in sqz_amd.__all__


def test_info_tool(lib, tmp_path, capsys):
    from sqz_amd import frame as F
    p = tmp_path / "f.sqzf"
    p.write_bytes(W.case_frame("laozi_w12_b12"))
    assert F.main(["info", str(p)]) == 0
    out = dict(line.split(": ") for line in capsys.readouterr().out.strip().splitlines())
    assert {k: int(v) for k, v in out.items()} == W.fields(W.case_frame("laozi_w12_b12"))
